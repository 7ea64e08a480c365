// mic.cc — fss_gates::MultipleIntervalContainmentGate
// (dcf/fss_gates/multiple_interval_containment.cc:37-308), the Fig. 14 gate
// of https://eprint.iacr.org/2020/1392, over the MI355X DCF.  Create and Gen
// are the reference's host logic, quirks included.  BatchEval uploads every
// key once and runs the fused gfx950 kernel (dpf_amd_mic_evaluate); the
// reference's strategy — two DCF BatchEvaluate calls over n * m replicated
// key pointers and a host combine — stays behind dpf_amd_set_mic_kernel(1).
#include "dpf_amd/multiple_interval_containment.h"

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "host_aes.h"
#include "host_device.h"

namespace distributed_point_functions {
namespace fss_gates {

using dpf_internal_host::AbiStatus;
using dpf_internal_host::CopyToHostSync;
using dpf_internal_host::DeviceBuffer;
using dpf_internal_host::ThreadStream;

namespace {

// The reference reads bounds and mask shares through value_uint128() only
// (cc:59-65, 157-163, 246-252, 297-298).  On a Value.Integer that carries
// value_uint64 that protobuf accessor returns the default Block, so such a
// value reads as 0 — kept, the contract is a drop-in.
uint128 Uint128Of(const Value::Integer& v) {
  if (!v.has_value_uint128()) return 0;
  return MakeUint128(v.value_uint128().high(), v.value_uint128().low());
}

void SetUint128(Value::Integer* v, uint128 x) {
  v->mutable_value_uint128()->set_high(Uint128High64(x));
  v->mutable_value_uint128()->set_low(Uint128Low64(x));
}

}  // namespace

MultipleIntervalContainmentGate::MultipleIntervalContainmentGate(
    MicParameters mic_parameters, std::unique_ptr<DistributedComparisonFunction> dcf)
    : mic_parameters_(std::move(mic_parameters)), dcf_(std::move(dcf)) {
  const uint128 N = uint128{1} << mic_parameters_.log_group_size();
  for (const Interval& iv : mic_parameters_.intervals()) {
    p_.push_back(Uint128Of(iv.lower_bound()));
    q_prime_.push_back((Uint128Of(iv.upper_bound()) + 1) % N);
  }
}

// cc:37-103.
StatusOr<std::unique_ptr<MultipleIntervalContainmentGate>> MultipleIntervalContainmentGate::Create(
    const MicParameters& mic_parameters) {
  if (mic_parameters.log_group_size() < 0 || mic_parameters.log_group_size() > 127)
    return InvalidArgumentError("log_group_size should be in > 0 and < 128");
  const uint128 N = uint128{1} << mic_parameters.log_group_size();
  for (int i = 0; i < mic_parameters.intervals_size(); ++i) {
    const Interval& iv = mic_parameters.intervals(i);
    if (!iv.has_lower_bound() || !iv.has_upper_bound())
      return InvalidArgumentError("Intervals should be non-empty");
    const uint128 p = Uint128Of(iv.lower_bound());
    const uint128 q = Uint128Of(iv.upper_bound());
    if (p >= N || q >= N)
      return InvalidArgumentError("Interval bounds should be between 0 and 2^log_group_size");
    if (p > q) return InvalidArgumentError("Interval upper bounds should be >= lower bound");
  }
  // A DCF over the gate's group with 128-bit outputs (cc:87-99); a
  // log_group_size of 0 fails here with the DCF's own message.
  DcfParameters dcf_parameters;
  dcf_parameters.mutable_parameters()->set_log_domain_size(mic_parameters.log_group_size());
  *dcf_parameters.mutable_parameters()->mutable_value_type() = ToValueType<uint128>();
  DPF_ASSIGN_OR_RETURN(std::unique_ptr<DistributedComparisonFunction> dcf,
                       DistributedComparisonFunction::Create(dcf_parameters));
  return std::unique_ptr<MultipleIntervalContainmentGate>(
      new MultipleIntervalContainmentGate(mic_parameters, std::move(dcf)));
}

// cc:110-209 (Fig. 14 Gen).
StatusOr<std::pair<MicKey, MicKey>> MultipleIntervalContainmentGate::GenImpl(
    uint128 r_in, const std::vector<uint128>& r_out, const uint128* seeds,
    const uint128* mask_shares) {
  const int m = mic_parameters_.intervals_size();
  if (static_cast<int64_t>(r_out.size()) != m)
    return InvalidArgumentError(
        "Count of output masks should be equal to the number of intervals");
  const uint128 N = uint128{1} << mic_parameters_.log_group_size();
  if (r_in >= N)
    return InvalidArgumentError("Input mask should be between 0 and 2^log_group_size");
  for (uint128 r : r_out)
    if (r >= N)
      return InvalidArgumentError("Output mask should be between 0 and 2^log_group_size");

  // Lines 1-2: a DCF key pair for (alpha = gamma, beta = 1).
  const uint128 gamma = (N - 1 + r_in) % N;
  const uint128 one = 1;
  StatusOr<std::pair<DcfKey, DcfKey>> dcf_keys =
      seeds ? dcf_->GenerateKeysWithSeeds(gamma, ToValue(one), seeds[0], seeds[1])
            : dcf_->GenerateKeys(gamma, one);
  if (!dcf_keys.ok()) return dcf_keys.status();
  std::pair<MicKey, MicKey> keys;
  *keys.first.mutable_dcfkey() = std::move(dcf_keys->first);
  *keys.second.mutable_dcfkey() = std::move(dcf_keys->second);

  for (int i = 0; i < m; ++i) {
    // Lines 3-4.
    const uint128 p = Uint128Of(mic_parameters_.intervals(i).lower_bound());
    const uint128 q = Uint128Of(mic_parameters_.intervals(i).upper_bound());
    const uint128 q_prime = (q + 1) % N;
    const uint128 alpha_p = (p + r_in) % N;
    const uint128 alpha_q = (q + r_in) % N;
    const uint128 alpha_q_prime = (q + 1 + r_in) % N;
    // Line 5 (Lemma 1, Lemma 2 and Theorem 3 of the paper): the -1 wraps in
    // uint128 and the final % N brings it back into the group.
    uint128 z = r_out[i] + (alpha_p > alpha_q ? 1 : 0) + (alpha_p > p ? ~uint128{0} : 0) +
                (alpha_q_prime > q_prime ? 1 : 0) + (alpha_q == (N - 1) ? 1 : 0);
    z = z % N;
    // Line 7: additive shares of z.
    uint128 z_0;
    if (mask_shares) {
      z_0 = mask_shares[i];
    } else if (!dpf_amd::SecureRandom(&z_0, sizeof(z_0))) {
      return InternalError("Failed to obtain random bytes");
    }
    z_0 = z_0 % N;
    const uint128 z_1 = (z - z_0) % N;
    SetUint128(keys.first.add_output_mask_share(), z_0);
    SetUint128(keys.second.add_output_mask_share(), z_1);
  }
  return keys;
}

StatusOr<std::pair<MicKey, MicKey>> MultipleIntervalContainmentGate::Gen(
    uint128 r_in, std::vector<uint128> r_out) {
  return GenImpl(r_in, r_out, nullptr, nullptr);
}

StatusOr<std::pair<MicKey, MicKey>> MultipleIntervalContainmentGate::GenWithSeeds(
    uint128 r_in, std::vector<uint128> r_out, uint128 seed0, uint128 seed1,
    Span<const uint128> mask_shares) {
  if (static_cast<int64_t>(mask_shares.size()) != mic_parameters_.intervals_size())
    return InvalidArgumentError(
        "Count of mask shares should be equal to the number of intervals");
  const uint128 seeds[2] = {seed0, seed1};
  return GenImpl(r_in, r_out, seeds, mask_shares.data());
}

StatusOr<std::vector<uint128>> MultipleIntervalContainmentGate::BatchEval(
    Span<const MicKey> keys, Span<const uint128> evaluation_points) {
  std::vector<const MicKey*> ptrs;
  ptrs.reserve(keys.size());
  for (const MicKey& k : keys) ptrs.push_back(&k);
  std::vector<uint128> res(keys.size() * static_cast<size_t>(num_intervals()));
  DPF_RETURN_IF_ERROR(BatchEvalRaw(Span<const MicKey* const>(ptrs.data(), ptrs.size()),
                                   evaluation_points, res.data()));
  return res;
}

// cc:211-308 (Fig. 14 Eval).
Status MultipleIntervalContainmentGate::BatchEvalRaw(Span<const MicKey* const> keys,
                                                     Span<const uint128> evaluation_points,
                                                     uint128* out) {
  if (keys.size() != evaluation_points.size())
    return InvalidArgumentError("`keys` and `evaluations_points` must have the same size");
  const uint128 N = uint128{1} << mic_parameters_.log_group_size();
  for (uint128 x : evaluation_points)
    if (x >= N)
      return InvalidArgumentError("Masked input should be between 0 and 2^log_group_size");
  const int m = num_intervals();
  if (m == 0 || keys.empty()) return OkStatus();
  for (const MicKey* k : keys) {
    DPF_RETURN_IF_ERROR(dcf_->dpf().ValidateKey(k->dcfkey().key()));
    // The reference indexes output_mask_share(j) unchecked (cc:297).
    if (k->output_mask_share_size() < m)
      return InvalidArgumentError(
          "MicKey has fewer output_mask_share entries than the gate has intervals");
  }
  return dpf_amd::MicKernelMode() == 1 ? EvalComposed(keys, evaluation_points, out)
                                       : EvalFused(keys, evaluation_points, out);
}

// The reference's evaluation, line by line: x_p / x_q' of every (key,
// interval), two DCF batch evaluations over replicated key pointers, line 7
// on the host.
Status MultipleIntervalContainmentGate::EvalComposed(Span<const MicKey* const> keys,
                                                     Span<const uint128> x, uint128* out) {
  const uint128 N = uint128{1} << mic_parameters_.log_group_size();
  const size_t n = keys.size(), m = static_cast<size_t>(num_intervals());
  std::vector<uint128> x_p(n * m), x_q_prime(n * m), s_p(n * m), s_q_prime(n * m);
  std::vector<const DcfKey*> dcf_keys(n * m);
  for (size_t i = 0; i < n; ++i)
    for (size_t j = 0; j < m; ++j) {
      x_p[i * m + j] = (x[i] + N - 1 - p_[j]) % N;  // line 4
      x_q_prime[i * m + j] = (x[i] + N - 1 - q_prime_[j]) % N;
      dcf_keys[i * m + j] = &keys[i]->dcfkey();
    }
  const dpf_amd_value_type layout = dpf_internal::HostLayoutOf<uint128>();
  const Span<const DcfKey* const> kp(dcf_keys.data(), dcf_keys.size());
  DPF_RETURN_IF_ERROR(dcf_->BatchEvaluateRaw(kp, x_p, layout, s_p.data()));              // line 5
  DPF_RETURN_IF_ERROR(dcf_->BatchEvaluateRaw(kp, x_q_prime, layout, s_q_prime.data()));  // line 6
  for (size_t i = 0; i < n; ++i)
    for (size_t j = 0; j < m; ++j) {
      const size_t index = i * m + j;
      const uint128 z = Uint128Of(keys[i]->output_mask_share(static_cast<int>(j)));
      const uint128 y = (keys[i]->dcfkey().key().party()
                             ? uint128{x[i] > p_[j]} - uint128{x[i] > q_prime_[j]}
                             : 0) -
                        s_p[index] % N + s_q_prime[index] % N + z;  // line 7
      out[index] = y % N;
    }
  return OkStatus();
}

// Every key's seed, control bit, party, correction words [tree level][n] and
// value corrections [hierarchy level][n] are uploaded once, with x[n],
// z[n][m], p[m] and q'[m]; one launch; n * m results come back.
Status MultipleIntervalContainmentGate::EvalFused(Span<const MicKey* const> keys,
                                                  Span<const uint128> x, uint128* out) {
  const DistributedPointFunction& dpf = dcf_->dpf();
  const int64_t n = static_cast<int64_t>(keys.size());
  const int64_t m = num_intervals();
  const int H = dpf.num_hierarchy_levels();
  const int L = dpf.hierarchy_to_tree(H - 1);
  // uint128 fills a block: hierarchy level h is tree level h, one element
  // and one correction per level.
  if (H != mic_parameters_.log_group_size() || L != H - 1)
    return InternalError("unexpected DCF tree shape");

  std::vector<uint128> seeds(n), cws(static_cast<size_t>(L) * n), corr(static_cast<size_t>(H) * n);
  std::vector<uint128> z(static_cast<size_t>(n) * m), tmp;
  std::vector<uint8_t> cbs(n), ccl(cws.size()), ccr(cws.size());
  std::vector<int8_t> party(n);
  for (int64_t i = 0; i < n; ++i) {
    const DpfKey& k = keys[i]->dcfkey().key();
    seeds[i] = MakeUint128(k.seed().high(), k.seed().low());
    cbs[i] = static_cast<uint8_t>(k.party() != 0);
    party[i] = static_cast<int8_t>(k.party());
    for (int a = 0; a < L; ++a) {
      const CorrectionWord& cw = k.correction_words(a);
      cws[a * n + i] = MakeUint128(cw.seed().high(), cw.seed().low());
      ccl[a * n + i] = cw.control_left();
      ccr[a * n + i] = cw.control_right();
    }
    for (int h = 0; h < H; ++h) {
      DPF_RETURN_IF_ERROR(dpf.ValueCorrectionWords(k, h, &tmp));
      if (tmp.size() != 1) return InternalError("value correction size");
      corr[static_cast<size_t>(h) * n + i] = tmp[0];
    }
    for (int64_t j = 0; j < m; ++j)
      z[i * m + j] = Uint128Of(keys[i]->output_mask_share(static_cast<int>(j)));
  }
  hipStream_t s = ThreadStream();
  DeviceBuffer dseeds, dcbs, dparty, dx, dcws, dccl, dccr, dcorr, dz, dp, dq, dout;
  DPF_RETURN_IF_ERROR(dseeds.Upload(seeds.data(), 16 * n, s));
  DPF_RETURN_IF_ERROR(dcbs.Upload(cbs.data(), n, s));
  DPF_RETURN_IF_ERROR(dparty.Upload(party.data(), n, s));
  DPF_RETURN_IF_ERROR(dx.Upload(x.data(), 16 * n, s));
  DPF_RETURN_IF_ERROR(dcws.Upload(cws.data(), 16 * cws.size(), s));
  DPF_RETURN_IF_ERROR(dccl.Upload(ccl.data(), ccl.size(), s));
  DPF_RETURN_IF_ERROR(dccr.Upload(ccr.data(), ccr.size(), s));
  DPF_RETURN_IF_ERROR(dcorr.Upload(corr.data(), 16 * corr.size(), s));
  DPF_RETURN_IF_ERROR(dz.Upload(z.data(), 16 * z.size(), s));
  DPF_RETURN_IF_ERROR(dp.Upload(p_.data(), 16 * m, s));
  DPF_RETURN_IF_ERROR(dq.Upload(q_prime_.data(), 16 * m, s));
  DPF_RETURN_IF_ERROR(dout.Alloc(16 * n * m, s));
  DPF_RETURN_IF_ERROR(AbiStatus(dpf_amd_mic_evaluate(
      n, m, H, dseeds.get(), dcbs.as<uint8_t>(), dparty.as<int8_t>(), dx.get(), dcws.get(),
      dccl.as<uint8_t>(), dccr.as<uint8_t>(), dcorr.get(), dz.get(), dp.get(), dq.get(),
      dout.get(), s)));
  return CopyToHostSync(out, dout.get(), 16 * n * m, s);
}

}  // namespace fss_gates
}  // namespace distributed_point_functions
