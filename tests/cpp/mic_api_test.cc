// mic_api_test.cc — the reference's fss_gates::MultipleIntervalContainmentGate
// used as a drop-in: written against include/dpf_amd/
// multiple_interval_containment.h as a caller of dcf/fss_gates/
// multiple_interval_containment.h would write it, and linked to
// libdpf_amd.so by plain g++.  Ports of multiple_interval_containment_test.cc:
//   :43-119  GenAndEvalSucceedsForSmallGroup,
//   :121-214 GenAndEvalSucceedsForLargeGroup,
//   :547-584 BatchEvalIsSameAsRepeatedEval.
// Exit status 0 = all checks passed.  Built by build_native and run by
// tests/test_mic_cpp.py.
#include <cstdio>
#include <memory>
#include <random>
#include <utility>
#include <vector>

#include "dpf_amd/multiple_interval_containment.h"

using namespace distributed_point_functions;
using namespace distributed_point_functions::fss_gates;

static int failures = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) {                                                                   \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                                    \
    }                                                                                \
  } while (0)
#define CHECK_OK(expr)                                                \
  do {                                                                \
    if (!(expr).ok()) {                                               \
      std::fprintf(stderr, "%s:%d: not OK: %s\n", __FILE__, __LINE__, \
                   (expr).status().ToString().c_str());               \
      return 1;                                                       \
    }                                                                 \
  } while (0)

static std::mt19937_64 rng(20201392);
static uint128 Rand128() { return MakeUint128(rng(), rng()); }

static void AddInterval(MicParameters* params, uint128 p, uint128 q) {
  Interval* interval = params->add_intervals();
  interval->mutable_lower_bound()->mutable_value_uint128()->set_high(Uint128High64(p));
  interval->mutable_lower_bound()->mutable_value_uint128()->set_low(Uint128Low64(p));
  interval->mutable_upper_bound()->mutable_value_uint128()->set_high(Uint128High64(q));
  interval->mutable_upper_bound()->mutable_value_uint128()->set_low(Uint128Low64(q));
}

// Gen with random masks, then both keys at x + r_in for every x of `xs`: the
// shares minus the output mask are 1 inside the interval and 0 outside.
static int GenAndEval(int log_group_size, const std::vector<uint128>& ps,
                      const std::vector<uint128>& qs, const std::vector<uint128>& xs,
                      bool masks_64_bit) {
  MicParameters mic_parameters;
  mic_parameters.set_log_group_size(log_group_size);
  for (size_t i = 0; i < ps.size(); ++i) AddInterval(&mic_parameters, ps[i], qs[i]);
  auto gate = MultipleIntervalContainmentGate::Create(mic_parameters);
  CHECK_OK(gate);
  const uint128 N = uint128{1} << mic_parameters.log_group_size();
  const uint128 r_in = (masks_64_bit ? uint128{rng()} : Rand128()) % N;
  std::vector<uint128> r_outs;
  for (size_t i = 0; i < ps.size(); ++i)
    r_outs.push_back((masks_64_bit ? uint128{rng()} : Rand128()) % N);
  auto keys = (*gate)->Gen(r_in, r_outs);
  CHECK_OK(keys);
  for (uint128 x : xs) {
    auto res_0 = (*gate)->Eval(keys->first, (x + r_in) % N);
    auto res_1 = (*gate)->Eval(keys->second, (x + r_in) % N);
    CHECK_OK(res_0);
    CHECK_OK(res_1);
    CHECK(res_0->size() == ps.size() && res_1->size() == ps.size());
    for (size_t j = 0; j < ps.size(); ++j) {
      const uint128 result = ((*res_0)[j] + (*res_1)[j] - r_outs[j]) % N;
      CHECK(result == ((x >= ps[j] && x <= qs[j]) ? 1 : 0));
    }
  }
  return 0;
}

static int GenAndEvalSucceedsForSmallGroup() {
  std::vector<uint128> xs;
  for (uint64_t i = 0; i < 400; ++i) xs.push_back(i);
  return GenAndEval(64, {10, 23, 45, 66, 15}, {45, 30, 100, 250, 15}, xs, true);
}

static int GenAndEvalSucceedsForLargeGroup() {
  const uint128 two_power_127 = uint128{1} << 127;
  const uint128 two_power_126 = uint128{1} << 126;
  return GenAndEval(
      127, {two_power_126, two_power_127 - 1, two_power_127 - 3},
      {two_power_126 + 3, two_power_127 - 1, two_power_127 - 2},
      {two_power_126 - 1, two_power_126, two_power_126 + 1, two_power_126 + 2, two_power_126 + 3,
       two_power_126 + 4, two_power_127 - 4, two_power_127 - 3, two_power_127 - 2,
       two_power_127 - 1},
      false);
}

static int BatchEvalIsSameAsRepeatedEval() {
  const int num_keys = 5, num_intervals = 7;
  MicParameters params;
  params.set_log_group_size(64);
  std::vector<MicKey> keys(num_keys);
  std::vector<uint128> evaluation_points(num_keys);
  std::vector<uint128> r_out(num_intervals);
  for (int i = 0; i < num_intervals; ++i) {
    uint64_t lower = rng(), upper = rng();
    if (lower > upper) std::swap(lower, upper);
    // As in the reference's test the bounds are set through value_uint64,
    // which the gate (reading value_uint128 only) sees as 0.
    Interval* interval = params.add_intervals();
    interval->mutable_lower_bound()->set_value_uint64(lower);
    interval->mutable_upper_bound()->set_value_uint64(upper);
    r_out[i] = rng();
  }
  auto gate = MultipleIntervalContainmentGate::Create(params);
  CHECK_OK(gate);
  for (int i = 0; i < num_keys; ++i) {
    auto k = (*gate)->Gen(uint128{rng()}, r_out);
    CHECK_OK(k);
    keys[i] = k->first;
  }
  auto evaluations = (*gate)->BatchEval(keys, evaluation_points);
  CHECK_OK(evaluations);
  std::vector<uint128> evaluations2;
  for (int i = 0; i < num_keys; ++i) {
    auto evaluations_i = (*gate)->Eval(keys[i], evaluation_points[i]);
    CHECK_OK(evaluations_i);
    evaluations2.insert(evaluations2.end(), evaluations_i->begin(), evaluations_i->end());
  }
  CHECK(evaluations->size() == static_cast<size_t>(num_keys * num_intervals));
  CHECK(*evaluations == evaluations2);
  return 0;
}

int main() {
  if (GenAndEvalSucceedsForSmallGroup() || GenAndEvalSucceedsForLargeGroup() ||
      BatchEvalIsSameAsRepeatedEval())
    return 1;
  if (failures) {
    std::fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
