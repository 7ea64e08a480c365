"""MultipleIntervalContainmentGate on the GPU (dcf/fss_gates/
multiple_interval_containment.cc:211-308, Fig. 14 Eval of eprint 2020/1392):
the fused kernel against the gate's semantics, against a Python restatement
of Eval over the oracle's DCF composition, and against the reference's own
strategy (two DCF batch evaluations combined on the host, dpf_amd_set_mic_
kernel(1)).  Every comparison is bit-exact.
"""
import random
import threading

import pytest

from distributed_point_functions_amd import kernels as K
from distributed_point_functions_amd.mic import (Interval, MicParameters,
                                                 MultipleIntervalContainmentGate)
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

SPEC = ("int", 128)
M128 = (1 << 128) - 1


def _gate(n, intervals):
    return MultipleIntervalContainmentGate.create(
        MicParameters(n, [Interval(p, q) for p, q in intervals]))


def _check_shares(N, intervals, r_out, xs, y0, y1):
    """(y0 + y1 - r_out) mod N == (p <= x <= q) for every (x, interval)."""
    m = len(intervals)
    assert len(y0) == len(y1) == len(xs) * m
    for i, x in enumerate(xs):
        for j, (p, q) in enumerate(intervals):
            got = (y0[i * m + j] + y1[i * m + j] - r_out[j]) % N
            assert got == int(p <= x <= q), (x, p, q)
            assert y0[i * m + j] < N and y1[i * m + j] < N


# ---------------------------------------------------------------------------
# Semantics
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("n,interior", [(1, (0, 1)), (2, (1, 2)), (4, (3, 9))])
def test_exhaustive_small_groups(cuda, n, interior):
    """Every input mask and every input, both parties, one batch_eval per
    party: log_group_size 1 has no correction words and one hierarchy level."""
    N = 1 << n
    intervals = [(0, 0), (0, N - 1), (N - 1, N - 1), interior]
    g = _gate(n, intervals)
    r_out = [(5 * j + 3) % N for j in range(len(intervals))]
    keys0, keys1, masked, xs = [], [], [], []
    for r_in in range(N):
        k0, k1 = g.gen(r_in, r_out, seeds=(2 * r_in + 1, 2 * r_in + 2),
                       mask_shares=[r_in + j for j in range(len(intervals))])
        for x in range(N):
            keys0.append(k0)
            keys1.append(k1)
            masked.append((x + r_in) % N)
            xs.append(x)
    _check_shares(N, intervals, r_out, xs, g.batch_eval(keys0, masked),
                  g.batch_eval(keys1, masked))


def test_gen_and_eval_succeeds_for_small_group(cuda):
    """GenAndEvalSucceedsForSmallGroup (multiple_interval_containment_test.cc:
    43-119): Z_{2^64}, 5 intervals, x in [0, 400)."""
    rng = random.Random(64)
    N = 1 << 64
    intervals = list(zip([10, 23, 45, 66, 15], [45, 30, 100, 250, 15]))
    g = _gate(64, intervals)
    r_in = rng.getrandbits(64)
    r_out = [rng.getrandbits(64) for _ in intervals]
    k0, k1 = g.gen(r_in, r_out)
    xs = list(range(400))
    masked = [(x + r_in) % N for x in xs]
    _check_shares(N, intervals, r_out, xs, g.batch_eval([k0] * 400, masked),
                  g.batch_eval([k1] * 400, masked))
    assert g.eval(k0, masked[17]) == g.batch_eval([k0] * 400, masked)[17 * 5:18 * 5]


def test_gen_and_eval_succeeds_for_large_group(cuda):
    """GenAndEvalSucceedsForLargeGroup (:121-214): Z_{2^127}, boundary points
    around 2^126 and 2^127 - 1."""
    rng = random.Random(127)
    N, A, B = 1 << 127, 1 << 126, 1 << 127
    intervals = [(A, A + 3), (B - 1, B - 1), (B - 3, B - 2)]
    xs = [A - 1, A, A + 1, A + 2, A + 3, A + 4, B - 4, B - 3, B - 2, B - 1]
    g = _gate(127, intervals)
    r_in = rng.getrandbits(128) % N
    r_out = [rng.getrandbits(128) % N for _ in intervals]
    k0, k1 = g.gen(r_in, r_out)
    masked = [(x + r_in) % N for x in xs]
    _check_shares(N, intervals, r_out, xs, g.batch_eval([k0] * len(xs), masked),
                  g.batch_eval([k1] * len(xs), masked))


def test_batch_eval_is_same_as_repeated_eval(cuda):
    """BatchEvalIsSameAsRepeatedEval (:547-584): 5 keys x 7 intervals at log 64."""
    rng = random.Random(547)
    intervals = [tuple(sorted((rng.getrandbits(64), rng.getrandbits(64)))) for _ in range(7)]
    r_out = [rng.getrandbits(64) for _ in range(7)]
    g = _gate(64, intervals)
    keys = [g.gen(rng.getrandbits(64), r_out)[0] for _ in range(5)]
    points = [0, 1, rng.getrandbits(64), intervals[0][0], intervals[1][1]]
    batched = g.batch_eval(keys, points)
    repeated = [y for k, x in zip(keys, points) for y in g.eval(k, x)]
    assert len(batched) == 35 and batched == repeated


# ---------------------------------------------------------------------------
# Per-party parity with the oracle's DCF composition
# ---------------------------------------------------------------------------

def _oracle_dcf_many(od, key, n, xs):
    """sum over h with bit (n - 1 - h) of x == 0 of EvaluateAt(key, h,
    x >> (n - h)) mod 2^128 (tests/test_dcf.py's _oracle_dcf), for many x,
    one oracle call per hierarchy level."""
    acc = [0] * len(xs)
    for h in range(n):
        idx = [i for i, x in enumerate(xs) if not (x >> (n - 1 - h)) & 1]
        if not idx:
            continue
        vals = od.evaluate_at(key, h, [xs[i] >> (n - h) for i in idx])
        for i, v in zip(idx, vals):
            acc[i] = (acc[i] + v[0]) & M128
    return acc


def _oracle_mic(od, okey, party, z, n, intervals, masked):
    """Fig. 14 Eval restated: key `okey` at the masked inputs."""
    N = 1 << n
    qp = [(q + 1) % N for _, q in intervals]
    pts_p = [(x + N - 1 - p) % N for x in masked for p, _ in intervals]
    pts_q = [(x + N - 1 - q) % N for x in masked for q in qp]
    s_p = _oracle_dcf_many(od, okey, n, pts_p)
    s_q = _oracle_dcf_many(od, okey, n, pts_q)
    out, m = [], len(intervals)
    for i, x in enumerate(masked):
        for j, (p, _) in enumerate(intervals):
            c = (int(x > p) - int(x > qp[j])) if party else 0
            out.append((c - s_p[i * m + j] % N + s_q[i * m + j] % N + z[j]) % N)
    return out


@pytest.mark.parametrize("n", [5, 33, 64, 127])
@pytest.mark.parametrize("m", [1, 7])
def test_each_party_matches_oracle_composition(cuda, n, m):
    """Distinct keys of both parties mixed in one batch, points at and next
    to every bound: each party's output alone equals Eval over the oracle."""
    rng = random.Random(1000 * n + m)
    N = 1 << n
    intervals = [(0, 0), (0, N - 1), (N - 1, N - 1)][:m]
    while len(intervals) < m:
        intervals.append(tuple(sorted((rng.randrange(N), rng.randrange(N)))))
    g = _gate(n, intervals)
    od = po.Dpf([(i, SPEC, 0) for i in range(n)])
    keys, masked, want = [], [], []
    for _ in range(3):
        r_in = rng.randrange(N)
        r_out = [rng.randrange(N) for _ in range(m)]
        seeds = (rng.getrandbits(128), rng.getrandbits(128))
        z0 = [rng.getrandbits(128) for _ in range(m)]
        mk = g.gen(r_in, r_out, seeds=seeds, mask_shares=z0)
        gamma = (N - 1 + r_in) % N
        ok = od.generate_keys(gamma >> 1, [1 if (gamma >> (n - 1 - i)) & 1 else 0
                                           for i in range(n)], seeds=seeds)
        xs = sorted({(b + d) % N for iv in intervals for b in iv for d in (-1, 0, 1)})
        for party in (0, 1):
            pts = [(x + r_in) % N for x in xs]
            keys += [mk[party]] * len(pts)
            masked += pts
            want += _oracle_mic(od, ok[party], party, mk[party].output_mask_share, n,
                                intervals, pts)
    assert g.batch_eval(keys, masked) == want


# ---------------------------------------------------------------------------
# Fused kernel == the reference's composition, launch shapes, threads
# ---------------------------------------------------------------------------

def _many_items(seed, n=16, m=7, gens=24, per_key=25):
    rng = random.Random(seed)
    N = 1 << n
    intervals = [(0, 0), (N - 1, N - 1)]
    while len(intervals) < m:
        intervals.append(tuple(sorted((rng.randrange(N), rng.randrange(N)))))
    g = _gate(n, intervals)
    r_out = [rng.randrange(N) for _ in range(m)]
    keys0, keys1, masked, xs = [], [], [], []
    for j in range(gens):
        r_in = rng.randrange(N)
        k0, k1 = g.gen(r_in, r_out, seeds=(2 * j + 11, 2 * j + 12),
                       mask_shares=[rng.getrandbits(128) for _ in range(m)])
        pts = [rng.randrange(N) for _ in range(per_key)] + [intervals[2][0], intervals[2][1]]
        keys0 += [k0] * len(pts)
        keys1 += [k1] * len(pts)
        xs += pts
        masked += [(x + r_in) % N for x in pts]
    return g, N, intervals, r_out, keys0, keys1, masked, xs


def test_fused_kernel_equals_composition(cuda):
    """A few thousand items over many waves and blocks, n * m not a multiple
    of 64, both parties: the fused kernel equals two DCF batch evaluations
    combined on the host, and the shares reconstruct the gate."""
    g, N, intervals, r_out, keys0, keys1, masked, xs = _many_items(16)
    keys0, keys1, masked, xs = keys0[:-1], keys1[:-1], masked[:-1], xs[:-1]
    assert len(masked) * 7 == 4529 and 4529 % 64 != 0
    with K.forced_mic_kernel(0):
        f0, f1 = g.batch_eval(keys0, masked), g.batch_eval(keys1, masked)
    with K.forced_mic_kernel(1):
        c0, c1 = g.batch_eval(keys0, masked), g.batch_eval(keys1, masked)
    assert f0 == c0 and f1 == c1
    _check_shares(N, intervals, r_out, xs, f0, f1)


@pytest.mark.parametrize("cap", [1, 3])
def test_more_items_than_the_grid_cap_holds(cuda, cap):
    """With the grid capped at `cap` blocks the lanes loop over the items:
    same result as the uncapped launch."""
    g, N, intervals, r_out, keys0, keys1, masked, xs = _many_items(7, gens=6, per_key=11)
    assert len(masked) * 7 == 546  # 64-thread blocks: 9 passes at cap 1, 3 at cap 3
    want0, want1 = g.batch_eval(keys0, masked), g.batch_eval(keys1, masked)
    with K.forced_mic_max_grid(cap):
        got0, got1 = g.batch_eval(keys0, masked), g.batch_eval(keys1, masked)
    assert got0 == want0 and got1 == want1
    _check_shares(N, intervals, r_out, xs, got0, got1)


def test_two_threads_share_a_gate(cuda):
    """Two Python threads call batch_eval on the same gate at once."""
    g, N, intervals, r_out, keys0, keys1, masked, xs = _many_items(3, gens=8, per_key=30)
    want = [g.batch_eval(keys0, masked), g.batch_eval(keys1, masked)]
    got, errors = [None, None], []

    def run(party, keys):
        try:
            for _ in range(4):
                got[party] = g.batch_eval(keys, masked)
                assert got[party] == want[party]
        except Exception as e:  # surfaced in the main thread
            errors.append(e)

    ts = [threading.Thread(target=run, args=(0, keys0)),
          threading.Thread(target=run, args=(1, keys1))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors and got == want
