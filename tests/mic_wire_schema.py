"""google.protobuf message classes for the MIC gate's wire schema
(dcf/fss_gates/multiple_interval_containment.proto: Interval, MicParameters,
MicKey in package distributed_point_functions.fss_gates), built from
descriptors in code on top of tests/wire_schema.py's pool - no .proto file or
protoc needed.  Test infrastructure: tests/golden/mic/make_mic.py and
tests/test_mic_cpu.py use these classes as the independent protobuf runtime
the hand-written codecs (csrc/wire.cc, distributed_point_functions_amd/mic.py)
must agree with byte for byte.
"""
from __future__ import annotations

from google.protobuf import descriptor_pb2, message_factory

from tests import wire_schema as W

PKG = W.PKG + ".fss_gates"


def _file():
    fd = descriptor_pb2.FileDescriptorProto(name="dpf_amd_mic_wire_schema.proto", package=PKG,
                                            syntax="proto3",
                                            dependency=["dpf_amd_wire_schema.proto"])
    fd.message_type.append(W._msg("Interval", [
        ("lower_bound", 1, W._MSG, W._OPT, W._t("Value.Integer"), None),
        ("upper_bound", 2, W._MSG, W._OPT, W._t("Value.Integer"), None)]))
    fd.message_type.append(W._msg("MicParameters", [
        ("log_group_size", 1, W._I32, W._OPT, None, None),
        ("intervals", 2, W._MSG, W._REP, "." + PKG + ".Interval", None)]))
    fd.message_type.append(W._msg("MicKey", [
        ("dcfkey", 1, W._MSG, W._OPT, W._t("DcfKey"), None),
        ("output_mask_share", 2, W._MSG, W._REP, W._t("Value.Integer"), None)]))
    return fd


W._POOL.Add(_file())


def cls(name: str):
    """Message class of Interval, MicParameters or MicKey."""
    return message_factory.GetMessageClass(W._POOL.FindMessageTypeByName(PKG + "." + name))


def set_uint128(msg, v: int):
    """A Value.Integer with value_uint128 set, as the reference's MIC code
    writes bounds and mask shares (set_high / set_low on the mutable Block)."""
    msg.value_uint128.SetInParent()
    msg.value_uint128.high = v >> 64
    msg.value_uint128.low = v & ((1 << 64) - 1)


def parameters(log_group_size: int, intervals):
    """MicParameters from (p, q) pairs; None leaves a bound unset."""
    m = cls("MicParameters")()
    m.log_group_size = log_group_size
    for p, q in intervals:
        iv = m.intervals.add()
        if p is not None:
            set_uint128(iv.lower_bound, p)
        if q is not None:
            set_uint128(iv.upper_bound, q)
    return m
