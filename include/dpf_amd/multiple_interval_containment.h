// multiple_interval_containment.h — the reference's
// fss_gates::MultipleIntervalContainmentGate
// (dcf/fss_gates/multiple_interval_containment.h:41-104), the Fig. 14 gate of
// https://eprint.iacr.org/2020/1392, on MI355X.  A gate over Z_{2^n} with m
// public intervals [p_j, q_j]: Gen makes two keys from an input mask and m
// output masks; evaluating a key at a masked input gives an additive share of
// m values, 1 where p_j <= x <= q_j and 0 elsewhere (plus the output mask).
// Create and Gen are the reference's host logic.  BatchEval runs as ONE fused
// gfx950 kernel (dpf_amd_mic_evaluate): every key is uploaded once, a lane
// walks an interval's two DCF points in lockstep and finishes Fig. 14 Eval
// line 7 in registers — instead of the reference's two DCF BatchEvaluate
// calls over n * m replicated key pointers and a host combine.
#ifndef DPF_AMD_MULTIPLE_INTERVAL_CONTAINMENT_H_
#define DPF_AMD_MULTIPLE_INTERVAL_CONTAINMENT_H_

#include <memory>
#include <utility>
#include <vector>

#include "dpf_amd/distributed_comparison_function.h"

namespace distributed_point_functions {
namespace fss_gates {

class MultipleIntervalContainmentGate {
 public:
  static StatusOr<std::unique_ptr<MultipleIntervalContainmentGate>> Create(
      const MicParameters& mic_parameters);

  MultipleIntervalContainmentGate(const MultipleIntervalContainmentGate&) = delete;
  MultipleIntervalContainmentGate& operator=(const MultipleIntervalContainmentGate&) = delete;

  // Keys for input mask `r_in` and one output mask per interval (Fig. 14 Gen).
  StatusOr<std::pair<MicKey, MicKey>> Gen(uint128 r_in, std::vector<uint128> r_out);
  // As Gen with explicit DCF root seeds and explicit party-0 mask shares z_0
  // (one per interval, reduced mod 2^n) instead of the CSPRNG (fixtures).
  StatusOr<std::pair<MicKey, MicKey>> GenWithSeeds(uint128 r_in, std::vector<uint128> r_out,
                                                   uint128 seed0, uint128 seed1,
                                                   Span<const uint128> mask_shares);

  // Key `k` at masked input `x`: one share per interval.
  StatusOr<std::vector<uint128>> Eval(const MicKey& k, uint128 x) {
    return BatchEval(Span<const MicKey>(&k, 1), Span<const uint128>(&x, 1));
  }

  // keys[i] at evaluation_points[i]; the share of key i and interval j is at
  // i * num_intervals + j.
  StatusOr<std::vector<uint128>> BatchEval(Span<const MicKey> keys,
                                           Span<const uint128> evaluation_points);
  // Raw entry (C ABI): writes keys.size() * num_intervals values to `out`.
  Status BatchEvalRaw(Span<const MicKey* const> keys, Span<const uint128> evaluation_points,
                      uint128* out);

  const MicParameters& parameters() const { return mic_parameters_; }
  int num_intervals() const { return mic_parameters_.intervals_size(); }

 private:
  MultipleIntervalContainmentGate(MicParameters mic_parameters,
                                  std::unique_ptr<DistributedComparisonFunction> dcf);
  StatusOr<std::pair<MicKey, MicKey>> GenImpl(uint128 r_in, const std::vector<uint128>& r_out,
                                              const uint128* seeds, const uint128* mask_shares);
  Status EvalFused(Span<const MicKey* const> keys, Span<const uint128> x, uint128* out);
  Status EvalComposed(Span<const MicKey* const> keys, Span<const uint128> x, uint128* out);

  const MicParameters mic_parameters_;
  std::unique_ptr<DistributedComparisonFunction> dcf_;
  // p_j, q'_j = (q_j + 1) mod N of every interval (Fig. 14 Eval lines 2-3).
  std::vector<uint128> p_, q_prime_;
};

}  // namespace fss_gates
}  // namespace distributed_point_functions

#endif  // DPF_AMD_MULTIPLE_INTERVAL_CONTAINMENT_H_
