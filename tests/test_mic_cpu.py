"""MultipleIntervalContainmentGate host logic (dcf/fss_gates/
multiple_interval_containment.cc): Create / Gen / BatchEval errors with the
reference's messages (multiple_interval_containment_test.cc:216-545), the
wire format of MicParameters / MicKey against the protobuf runtime
(tests/mic_wire_schema.py, fixtures of tests/golden/mic/make_mic.py), and
Fig. 14 Gen checked term by term.  No GPU: every check here ends before a
launch.
"""
import ctypes
import json
import os

import pytest

from distributed_point_functions_amd import _lib, wire
from distributed_point_functions_amd import value_types as V
from distributed_point_functions_amd._lib import DpfAmdError
from distributed_point_functions_amd.dcf import DcfParameters, DistributedComparisonFunction
from distributed_point_functions_amd.dpf import DpfParameters
from distributed_point_functions_amd.mic import (Interval, MicKey, MicParameters,
                                                 MultipleIntervalContainmentGate)
from tests import mic_wire_schema as MW

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mic")
GOLDEN = json.load(open(os.path.join(HERE, "mic.json")))


def _gate(log_group_size, intervals):
    return MultipleIntervalContainmentGate.create(
        MicParameters(log_group_size, [Interval(p, q) for p, q in intervals]))


def _fails(fn, message):
    with pytest.raises(DpfAmdError) as e:
        fn()
    assert e.value.code == 3 and e.value.message == message, e.value.message


def _case(name):
    c = GOLDEN[name]
    return dict(n=c["log_group_size"], intervals=[(int(p), int(q)) for p, q in c["intervals"]],
                r_in=int(c["r_in"]), r_out=[int(r) for r in c["r_out"]],
                seeds=tuple(int(s) for s in c["seeds"]), z0=[int(z) for z in c["z0"]],
                parameters=bytes.fromhex(c["parameters"]),
                keys=[bytes.fromhex(k) for k in c["keys"]])


# ---------------------------------------------------------------------------
# Create
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("log_group_size", [128, 129, -1])
def test_create_fails_outside_0_127(log_group_size):
    """CreateFailsWith128bitGroup (:216-242)."""
    _fails(lambda: _gate(log_group_size, [(0, 1)]), "log_group_size should be in > 0 and < 128")


def test_create_with_log_group_size_0_fails_in_the_dcf():
    """0 passes the gate's own range check (cc:43) and fails in the DCF."""
    _fails(lambda: _gate(0, [(0, 0)]), "A DCF must have log_domain_size >= 1")


@pytest.mark.parametrize("p,q", [(0, 1024), (1024, 1024), (3, 1 << 100)])
def test_create_fails_for_bounds_outside_group(p, q):
    """CreateFailsForIntervalBoundariesOutsideGroup (:244-271): a bound equal
    to N is outside."""
    _fails(lambda: _gate(10, [(1, 2), (p, q)]),
           "Interval bounds should be between 0 and 2^log_group_size")


def test_create_fails_for_lower_above_upper():
    """CreateFailsForInvalidIntervalBoundaries (:273-299)."""
    _fails(lambda: _gate(10, [(5, 4)]), "Interval upper bounds should be >= lower bound")


@pytest.mark.parametrize("p,q", [(None, 5), (5, None), (None, None)])
def test_create_fails_for_missing_bound(p, q):
    """CreateFailsForEmptyInterval (:301-324): has_lower_bound / has_upper_bound
    are observable."""
    _fails(lambda: _gate(10, [(0, 3), (p, q)]), "Intervals should be non-empty")


def test_create_reads_uint64_bounds_as_zero():
    """Bounds are read through value_uint128 only: a Value.Integer carrying
    value_uint64 reads as 0 (the protobuf accessor on the other oneof case),
    so lower 9 / upper 3 given as uint64 is the valid interval [0, 0]."""
    iv = (wire.field_message(1, wire.field_varint(1, 9)) +
          wire.field_message(2, wire.field_varint(1, 3)))
    proto = wire.field_varint(1, 10) + wire.field_message(2, iv)
    h = ctypes.c_void_p()
    assert _lib.lib().dpf_amd_mic_create(proto, len(proto), ctypes.byref(h)) == 0
    _lib.lib().dpf_amd_mic_destroy(h)


def test_create_fails_for_malformed_parameters():
    proto = wire.field_varint(1, 10) + b"\x12\x7f\x00"  # intervals length past the end
    h = ctypes.c_void_p()
    assert _lib.lib().dpf_amd_mic_create(proto, len(proto), ctypes.byref(h)) == 3
    assert _lib.lib().dpf_amd_last_error().decode() == "malformed MicParameters proto"


def test_create_without_intervals_evaluates_to_nothing():
    """Zero intervals: Create succeeds (cc:52 loops over none) and BatchEval
    returns an empty result without a launch."""
    g = _gate(10, [])
    k0, k1 = g.gen(5, [])
    assert k0.output_mask_share == [] and g.batch_eval([k0, k1], [1, 2]) == []
    assert _gate(10, [(1, 2)]).batch_eval([], []) == []


# ---------------------------------------------------------------------------
# Gen / BatchEval errors
# ---------------------------------------------------------------------------

def test_gen_fails_for_wrong_number_of_output_masks():
    """GenFailsForIncorrectNumberOfOutputMasks (:326-380)."""
    g = _gate(64, [(10, 45), (23, 30), (45, 100)])
    for r_out in ([1, 2], [1, 2, 3, 4], []):
        _fails(lambda: g.gen(7, r_out),
               "Count of output masks should be equal to the number of intervals")


def test_gen_fails_for_masks_outside_group():
    """GenFailsForInputMaskOutsideGroup / ...OutputMask... (:382-488): 2048
    at log_group_size 10."""
    g = _gate(10, [(10, 45), (23, 30)])
    _fails(lambda: g.gen(2048, [1, 2]), "Input mask should be between 0 and 2^log_group_size")
    _fails(lambda: g.gen(1024, [1, 2]), "Input mask should be between 0 and 2^log_group_size")
    _fails(lambda: g.gen(5, [1, 2048]), "Output mask should be between 0 and 2^log_group_size")


def test_batch_eval_fails_for_masked_input_outside_group():
    """EvalFailsForMaskedInputOutsideGroup (:490-545): 2^72 at log 64."""
    g = _gate(64, [(10, 45)])
    k0, _ = g.gen(3, [4], seeds=(1, 2), mask_shares=[9])
    _fails(lambda: g.eval(k0, 1 << 72),
           "Masked input should be between 0 and 2^log_group_size")
    _fails(lambda: g.batch_eval([k0, k0], [5, 1 << 64]),
           "Masked input should be between 0 and 2^log_group_size")


def test_batch_eval_fails_for_mismatched_sizes():
    g = _gate(64, [(10, 45)])
    k0, _ = g.gen(3, [4], seeds=(1, 2), mask_shares=[9])
    for keys, pts in (([k0], [1, 2]), ([k0, k0], [1]), ([], [1])):
        _fails(lambda: g.batch_eval(keys, pts),
               "`keys` and `evaluations_points` must have the same size")


def test_batch_eval_fails_for_key_with_too_few_mask_shares():
    """The one deliberate addition: the reference would index
    output_mask_share(j) out of range (cc:297)."""
    g3 = _gate(16, [(1, 2), (3, 4), (5, 6)])
    g2 = _gate(16, [(1, 2), (3, 4)])
    k0, _ = g2.gen(3, [4, 5], seeds=(1, 2), mask_shares=[9, 8])
    _fails(lambda: g3.eval(k0, 7),
           "MicKey has fewer output_mask_share entries than the gate has intervals")


def test_batch_eval_fails_for_invalid_and_malformed_keys():
    g = _gate(16, [(1, 2)])
    with pytest.raises(DpfAmdError) as e:  # an empty DpfKey: the DPF's own ValidateKey
        g.eval(MicKey(b""), 7)
    assert e.value.code == 3 and "key" in e.value.message.lower()
    _fails(lambda: g.eval(_raw(b"\x0a\x7f"), 7), "malformed MicKey proto")  # length past the end


def _raw(data):
    """A MicKey object around bytes the Python decoder would refuse."""
    k = MicKey.__new__(MicKey)
    k.data = data
    return k


# ---------------------------------------------------------------------------
# Wire format
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_parameters_serialize_like_protobuf(name):
    c = _case(name)
    ours = MicParameters(c["n"], [Interval(p, q) for p, q in c["intervals"]]).to_proto()
    assert ours == c["parameters"]
    m = MW.cls("MicParameters")()
    m.ParseFromString(ours)
    assert m.log_group_size == c["n"]
    assert [(wire.decode_block(iv.lower_bound.value_uint128.SerializeToString()),
             wire.decode_block(iv.upper_bound.value_uint128.SerializeToString()))
            for iv in m.intervals] == c["intervals"]
    # the native parser accepts the protobuf bytes
    h = ctypes.c_void_p()
    assert _lib.lib().dpf_amd_mic_create(c["parameters"], len(c["parameters"]),
                                         ctypes.byref(h)) == 0
    _lib.lib().dpf_amd_mic_destroy(h)


def test_unset_and_zero_bounds_serialize_like_protobuf():
    """An unset bound is absent, a zero bound is an empty value_uint128."""
    for intervals in ([(None, 5)], [(0, None)], [(0, 0)], [(None, None)]):
        ours = MicParameters(7, [Interval(p, q) for p, q in intervals]).to_proto()
        assert ours == MW.parameters(7, intervals).SerializeToString(deterministic=True)
    assert MicParameters(0, []).to_proto() == MW.parameters(0, []).SerializeToString()
    assert MicParameters(-1, []).to_proto() == MW.parameters(-1, []).SerializeToString()


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_seeded_gen_serializes_like_protobuf_and_parses_back(name):
    """The native Gen with the fixture's seeds and mask shares writes the
    bytes the protobuf runtime wrote for the same messages, and the Python
    mirror reads them back."""
    c = _case(name)
    g = _gate(c["n"], c["intervals"])
    keys = g.gen(c["r_in"], c["r_out"], seeds=c["seeds"], mask_shares=c["z0"])
    N = 1 << c["n"]
    for party, (k, golden) in enumerate(zip(keys, c["keys"])):
        assert bytes(k) == golden
        assert MW.cls("MicKey").FromString(golden).SerializeToString(deterministic=True) == golden
        back = MicKey(golden)
        assert back == k and back.dcfkey.key.party == party
        assert len(back.output_mask_share) == len(c["intervals"])
    assert keys[0].output_mask_share == [z % N for z in c["z0"]]


def test_every_truncation_of_a_key_parses_or_is_refused():
    """Each prefix of a golden MicKey either parses or returns the
    malformed-proto error (a gate without intervals returns before any
    launch, so this runs without a GPU)."""
    golden = _case("log10")["keys"][0]
    g = _gate(10, [])
    outcomes = set()
    for cut in range(len(golden) + 1):
        try:
            assert g.batch_eval([_raw(golden[:cut])], [0]) == []
            outcomes.add("parsed")
        except DpfAmdError as e:
            assert e.code == 3 and e.message == "malformed MicKey proto", (cut, e.message)
            outcomes.add("refused")
    assert outcomes == {"parsed", "refused"}


# ---------------------------------------------------------------------------
# Gen
# ---------------------------------------------------------------------------

def _line5(N, p, q, r_in, r_out):
    q_prime = (q + 1) % N
    alpha_p, alpha_q, alpha_q_prime = (p + r_in) % N, (q + r_in) % N, (q + 1 + r_in) % N
    return (r_out + (alpha_p > alpha_q) - (alpha_p > p) + (alpha_q_prime > q_prime)
            + (alpha_q == N - 1)) % N


# (log_group_size, intervals, r_in): together they reach every term of line 5
GEN_CASES = [
    (10, [(100, 200)], 900),            # alpha_p > alpha_q: the mask wraps inside the interval
    (10, [(100, 200)], 823),            # alpha_q = N - 1
    (10, [(7, 1023)], 5),               # q = N - 1, so q' = 0
    (10, [(0, 50)], 0),                 # p = 0, r_in = 0: alpha_p = p
    (10, [(0, 50)], 1023),              # p = 0, alpha_p > p
    (10, [(33, 33)], 990),              # p = q
    (10, [(33, 33)], 991),              # p = q, alpha_p wraps to 0
    (10, [(0, 0), (0, 1023), (1023, 1023), (5, 6)], 1),
    (1, [(0, 0), (0, 1), (1, 1)], 1),
    (64, [(10, 45), (0, (1 << 64) - 1)], (1 << 64) - 20),
    (127, [(1 << 126, (1 << 127) - 1)], (1 << 126) + 1),
]


@pytest.mark.parametrize("n,intervals,r_in", GEN_CASES)
def test_seeded_gen_follows_fig14(n, intervals, r_in):
    N = 1 << n
    m = len(intervals)
    g = _gate(n, intervals)
    r_out = [(0x9E3779B97F4A7C15 * (j + 1) * (r_in + 3)) % N for j in range(m)]
    z0 = [((1 << 127) - 1 - 977 * j) for j in range(m)]  # reduced mod N by Gen
    seeds = (r_in * 2 + 1, (1 << 100) + n)
    k0, k1 = g.gen(r_in, r_out, seeds=seeds, mask_shares=z0)
    dcf = DistributedComparisonFunction.create(DcfParameters(DpfParameters(n, V.Integer(128))))
    d0, d1 = dcf.generate_keys((N - 1 + r_in) % N, 1, seeds=seeds)
    assert bytes(k0.dcfkey) == bytes(d0) and bytes(k1.dcfkey) == bytes(d1)
    assert k0.output_mask_share == [z % N for z in z0]
    want = [_line5(N, p, q, r_in, r) for (p, q), r in zip(intervals, r_out)]
    assert [(a + b) % N for a, b in zip(k0.output_mask_share, k1.output_mask_share)] == want
    assert all(z < N for z in k1.output_mask_share)


def test_gen_cases_reach_every_term_of_line5():
    """The cases above are not vacuous: each comparison of line 5 is true in
    one and false in another."""
    seen = set()
    for n, intervals, r_in in GEN_CASES:
        N = 1 << n
        for p, q in intervals:
            ap, aq, aqp, qp = (p + r_in) % N, (q + r_in) % N, (q + 1 + r_in) % N, (q + 1) % N
            seen |= {("wrap", ap > aq), ("ap>p", ap > p), ("aq'>q'", aqp > qp),
                     ("aq=N-1", aq == N - 1), ("q'=0", qp == 0), ("p=0", p == 0), ("p=q", p == q)}
    assert all((t, b) in seen for t in ("wrap", "ap>p", "aq'>q'", "aq=N-1", "q'=0", "p=0", "p=q")
               for b in (True, False))


def test_unseeded_gen_draws_fresh_shares():
    g = _gate(64, [(10, 45), (23, 30)])
    a0, a1 = g.gen(7, [1, 2])
    b0, b1 = g.gen(7, [1, 2])
    assert a0.output_mask_share != b0.output_mask_share
    assert bytes(a0.dcfkey) != bytes(b0.dcfkey)
    N = 1 << 64
    for k0, k1 in ((a0, a1), (b0, b1)):  # both still share line 5's z
        assert [(x + y) % N for x, y in zip(k0.output_mask_share, k1.output_mask_share)] == \
            [_line5(N, p, q, 7, r) for (p, q), r in zip([(10, 45), (23, 30)], [1, 2])]


def test_gen_needs_seeds_and_mask_shares_together():
    g = _gate(10, [(1, 2)])
    with pytest.raises(ValueError):
        g.gen(1, [2], seeds=(1, 2))
    with pytest.raises(ValueError):
        g.gen(1, [2], mask_shares=[3])


def test_mic_hooks_validate_and_are_per_thread():
    """dpf_amd_set_mic_kernel (0 / 1) and dpf_amd_set_mic_max_grid refuse
    invalid values unchanged and are per thread."""
    import threading
    L = _lib.lib()
    assert L.dpf_amd_set_mic_kernel(2) == -2 and L.dpf_amd_set_mic_kernel(-1) == -2
    assert L.dpf_amd_set_mic_max_grid(-1) == -2 and L.dpf_amd_set_mic_max_grid(65537) == -2
    assert L.dpf_amd_set_mic_kernel(1) == 0
    assert L.dpf_amd_set_mic_max_grid(3) == 0
    seen = {}

    def other():
        seen["mode"] = L.dpf_amd_set_mic_kernel(0)
        seen["grid"] = L.dpf_amd_set_mic_max_grid(0)

    t = threading.Thread(target=other)
    t.start()
    t.join()
    assert seen == {"mode": 0, "grid": 0}
    assert L.dpf_amd_set_mic_kernel(0) == 1
    assert L.dpf_amd_set_mic_max_grid(0) == 3
