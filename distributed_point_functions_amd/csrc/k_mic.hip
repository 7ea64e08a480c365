// k_mic.hip — fused Multiple Interval Containment gate evaluation
// (dcf/fss_gates/multiple_interval_containment.cc:211-308, Fig. 14 Eval of
// https://eprint.iacr.org/2020/1392).
//
// One work item is (key i, interval j).  Its lane walks the two DCF points
// x_p = x - 1 - p_j and x_q' = x - 1 - q'_j (mod N) down key i's tree in
// lockstep: both chains belong to the same key, so a level's correction word
// is loaded once and serves both, and the two AES chains keep the LDS fed as
// the two points of KEvaluatePoints do.  Consecutive lanes hold consecutive
// intervals of one key, so a wave's correction-word loads mostly broadcast.
// The DCF sums (dcf/distributed_comparison_function.h:141-187) and line 7 of
// Eval stay in registers; only the n * m results are written.
#include "aes_device.h"
#include "walk_device.h"

namespace dpf_amd {

// Blocks of a launch: past one resident round (2 blocks per CU) the
// dispatcher back-fills CUs that finish early; lanes loop over the items
// beyond the cap.
#ifndef DPF_MIC_MAX_GRID
#define DPF_MIC_MAX_GRID 2048
#endif
// Queued value hashes per lane (0: hashed in place at every level).  2^16
// keys x 10 intervals at log_group_size 64: 1.88 / 1.72 / 1.63 ms at 0 / 4 /
// 6 (89 / 109 / 119 VGPRs, no scratch); 8 would not fit 4 waves/SIMD.
#ifndef DPF_MIC_QUEUE
#define DPF_MIC_QUEUE 6
#endif

__device__ __forceinline__ u128 U128Of(const uint4& v) {
  return (u128)v.x | ((u128)v.y << 32) | ((u128)v.z << 64) | ((u128)v.w << 96);
}

// Two chains per lane: the register budget of KEvaluatePoints' two-point
// path (4 waves/SIMD, two 64 KiB-table blocks per CU).
__global__ __launch_bounds__(kPointsBlock, kPointsWaves) void KMicEvaluate(MicArgs a) {
  __shared__ uint32_t tab[kTabWords];
  FillTables(tab);
  __syncthreads();
  const Lds L = MakeLds(tab);
  const int64_t T = (int64_t)gridDim.x * blockDim.x;
  const int64_t total = a.n * a.m;
  const int H = a.log_group_size;  // hierarchy levels; level h is tree level h
  const u128 group_mask = (((u128)1 << (H - 1)) << 1) - 1;  // N - 1, H in [1, 128)
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += T) {
    const int64_t i = idx / a.m;
    const int64_t j = idx - i * a.m;
    uint4 pt[2];  // the chains' points: x_p, x_q'
    {
      const u128 x = U128Of(a.x[i]);
      const u128 xp = (x - 1 - U128Of(a.p[j])) & group_mask;
      const u128 xq = (x - 1 - U128Of(a.q_prime[j])) & group_mask;
      pt[0] = make_uint4((uint32_t)xp, (uint32_t)(xp >> 32), (uint32_t)(xp >> 64),
                         (uint32_t)(xp >> 96));
      pt[1] = make_uint4((uint32_t)xq, (uint32_t)(xq >> 32), (uint32_t)(xq >> 64),
                         (uint32_t)(xq >> 96));
    }
    const uint4 s0 = a.seeds[i];
    uint32_t x[2][4] = {{s0.x, s0.y, s0.z, s0.w}, {s0.x, s0.y, s0.z, s0.w}};
    uint32_t t[2];
    t[0] = t[1] = a.cb[i];
    const bool negate = a.party[i] == 1;
    u128 acc[2] = {0, 0};  // s_p, s_q'
#if DPF_MIC_QUEUE > 0
    // A chain needs the value hash of about half its levels; hashing in place
    // runs both chains' hashes at every level some lane needs one.  Here a
    // lane queues the seeds it needs (KDcfEvaluateDirect's DPF_DCF_QUEUE, two
    // chains wide) and the wave hashes two queued seeds per lane at a time.
    // + mod 2^128 is commutative, so the order does not change the sums.
    constexpr int KQ = DPF_MIC_QUEUE;
    static_assert(KQ >= 4, "a level queues up to two seeds on top of one left over");
    uint32_t qx[KQ][4] = {}, qm[KQ] = {};
    int cnt = 0;
    auto pop2 = [&]() {
      const uint32_t xs[2][4] = {{qx[0][0], qx[0][1], qx[0][2], qx[0][3]},
                                 {qx[1][0], qx[1][1], qx[1][2], qx[1][3]}};
      u128 W[2][1];
      HashSeeds<2, 1>(xs, W, L);
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        if (cnt > c) {
          const int hh = (int)(qm[c] & 255u);
          u128 v = W[c][0];
          if (qm[c] >> 9) v += U128Of(a.corrections[(int64_t)hh * a.n + i]);
          if (negate) v = 0 - v;
          if ((qm[c] >> 8) & 1u)
            acc[1] += v;
          else
            acc[0] += v;
        }
      }
#pragma unroll
      for (int k = 0; k + 2 < KQ; ++k) {
#pragma unroll
        for (int w = 0; w < 4; ++w) qx[k][w] = qx[k + 2][w];
        qm[k] = qm[k + 2];
      }
      cnt = cnt > 2 ? cnt - 2 : 0;
    };
#endif
    for (int h = 0; h < H; ++h) {
      if (DPF_DCF_PRIO) WalkPrio(h, H);
      if (h > 0) {
        // tree level h - 1 of both chains off one correction word
        const Cw cw = LoadCw(a.cw_seed, a.ccl, a.ccr, (int64_t)(h - 1) * a.n + i);
        uint32_t bit[2], sg[2][4], st[2][4];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          bit[c] = PathBit(pt[c], H - h);
          Sigma(x[c], sg[c]);
#pragma unroll
          for (int w = 0; w < 4; ++w) st[c][w] = sg[c][w];
        }
        AesN<2>(st, DpfMasked<2>{{0u - bit[0], 0u - bit[1]}}, L);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const uint32_t m = 0u - t[c];
#pragma unroll
          for (int w = 0; w < 4; ++w) x[c][w] = st[c][w] ^ sg[c][w] ^ (cw.seed[w] & m);
          const uint32_t nt = (x[c][0] & 1u) ^ (t[c] & (bit[c] ? cw.cr : cw.cl));
          x[c][0] &= ~1u;
          t[c] = nt;
        }
      }
      // Level h's value counts where bit (H - 1 - h) of the chain's point is
      // 0 (h:150-165): element 0 of the block, corrected when the control
      // bit is set, negated for party 1.
      const bool need0 = PathBit(pt[0], H - 1 - h) == 0;
      const bool need1 = PathBit(pt[1], H - 1 - h) == 0;
#if DPF_MIC_QUEUE > 0
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        if (c == 0 ? need0 : need1) {
#pragma unroll
          for (int k = 0; k < KQ; ++k)
            if (cnt == k) {
#pragma unroll
              for (int w = 0; w < 4; ++w) qx[k][w] = x[c][w];
              qm[k] = (uint32_t)h | ((uint32_t)c << 8) | (t[c] << 9);
            }
          ++cnt;
        }
      }
      // wave-uniform: hash two queued seeds per lane while every active lane
      // holds two, or some lane has no room for the next level's two
      while (__builtin_amdgcn_ballot_w64(cnt < 2) == 0 ||
             __builtin_amdgcn_ballot_w64(cnt > KQ - 2) != 0)
        pop2();
#else
      if (__builtin_amdgcn_ballot_w64(need0 || need1) == 0) continue;  // wave-uniform
      u128 W[2][1];
      HashSeeds<2, 1>(x, W, L);
      const u128 corr = U128Of(a.corrections[(int64_t)h * a.n + i]);
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        u128 v = W[c][0];
        if (t[c]) v += corr;
        if (negate) v = 0 - v;
        if (c == 0 ? need0 : need1) acc[c] += v;
      }
#endif
    }
#if DPF_MIC_QUEUE > 0
    while (__builtin_amdgcn_ballot_w64(cnt > 0) != 0) pop2();
#endif
    // Fig. 14 Eval line 7; N divides 2^128, so one final mask equals the
    // reference's intermediate % N steps.
    const u128 xv = U128Of(a.x[i]);
    u128 y = U128Of(a.z[idx]) - acc[0] + acc[1];
    if (a.party[i] != 0)
      y += (u128)(xv > U128Of(a.p[j]) ? 1 : 0) - (u128)(xv > U128Of(a.q_prime[j]) ? 1 : 0);
    y &= group_mask;
    a.out[idx] = make_uint4((uint32_t)y, (uint32_t)(y >> 32), (uint32_t)(y >> 64),
                            (uint32_t)(y >> 96));
  }
}

int LaunchMicEvaluate(hipStream_t st, const MicArgs& a) {
  const int64_t total = a.n * a.m;
  const int block = WalkBlock(total, kPointsBlock);
  const int cap = MicMaxGrid() > 0 ? MicMaxGrid() : DPF_MIC_MAX_GRID;
  const int grid = (int)std::min<int64_t>(cap, (total + block - 1) / block);
  hipLaunchKernelGGL(KMicEvaluate, dim3(grid), dim3(block), 0, st, a);
  return LaunchCheck("mic kernel launch");
}

}  // namespace dpf_amd
