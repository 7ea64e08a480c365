"""Python mirror of the reference's fss_gates::MultipleIntervalContainmentGate
(dcf/fss_gates/multiple_interval_containment.h:41-104), the Fig. 14 gate of
https://eprint.iacr.org/2020/1392, over the Tier-2 C ABI.

A gate over Z_{2^n} with m public intervals [p_j, q_j]: gen() makes two keys
from an input mask r_in and m output masks; evaluating a key at the masked
input x + r_in gives an additive share (mod 2^n) of r_out[j] + (p_j <= x <=
q_j) per interval.  batch_eval runs as one fused gfx950 kernel.  Keys travel
as serialized MicKey protos; errors raise DpfAmdError with the reference's
status code and message.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

from . import _lib, wire
from ._lib import check, take_buffer
from .dcf import DcfKey
from .dpf import _seq
from .value_types import u128_words

MASK64 = (1 << 64) - 1


def _value_uint128(v: int) -> bytes:
    """Value.Integer with value_uint128 set, as the reference's MIC code
    writes bounds and mask shares (a set oneof member is always written)."""
    return wire.field_message(2, wire.block(v))


def _read_value_uint128(data: bytes) -> int:
    """value_uint128() of a Value.Integer: 0 when the message carries
    value_uint64 instead (the accessor on the other oneof case)."""
    d = wire.decode(data)
    return wire.decode_block(d[2][-1]) if 2 in d else 0


@dataclass
class Interval:
    """Interval proto (multiple_interval_containment.proto): bounds are
    Value.Integer with value_uint128 set; None leaves the bound unset."""

    lower_bound: Optional[int] = None
    upper_bound: Optional[int] = None

    def to_proto(self) -> bytes:
        out = b""
        if self.lower_bound is not None:
            out += wire.field_message(1, _value_uint128(self.lower_bound))
        if self.upper_bound is not None:
            out += wire.field_message(2, _value_uint128(self.upper_bound))
        return out


@dataclass
class MicParameters:
    """MicParameters proto: log_group_size = 1, repeated intervals = 2."""

    log_group_size: int
    intervals: List[Interval] = field(default_factory=list)

    def to_proto(self) -> bytes:
        out = b""
        if self.log_group_size:
            out += wire.field_varint(1, self.log_group_size)
        for iv in self.intervals:
            out += wire.field_message(2, iv.to_proto())
        return out


class MicKey:
    """A serialized MicKey proto; `.dcfkey` is the DcfKey and
    `.output_mask_share` the per-interval shares (value_uint128)."""

    def __init__(self, data: bytes):
        self.data = bytes(data)
        d = wire.decode(self.data)
        self.dcfkey = DcfKey(d[1][-1]) if 1 in d else DcfKey(b"")
        self.output_mask_share = [_read_value_uint128(v) for v in d.get(2, [])]

    def __bytes__(self):
        return self.data

    def __eq__(self, other):
        return isinstance(other, MicKey) and self.data == other.data


def _words_ptr(values, count):
    w = u128_words(_seq(values)) if count else np.zeros(2, np.uint64)
    return w, w.ctypes.data_as(ctypes.c_void_p)


class MultipleIntervalContainmentGate:
    """MultipleIntervalContainmentGate (multiple_interval_containment.h:41)."""

    def __init__(self, handle, parameters: MicParameters):
        self._h = handle
        self.parameters = parameters

    def __del__(self):
        try:
            if self._h:
                _lib.lib().dpf_amd_mic_destroy(self._h)
        except Exception:
            pass

    @classmethod
    def create(cls, parameters: MicParameters) -> "MultipleIntervalContainmentGate":
        data = parameters.to_proto()
        h = ctypes.c_void_p()
        check(_lib.lib().dpf_amd_mic_create(data, len(data), ctypes.byref(h)))
        return cls(h, parameters)

    @property
    def num_intervals(self) -> int:
        return len(self.parameters.intervals)

    def gen(self, r_in: int, r_out: Sequence[int], seeds: Optional[Sequence[int]] = None,
            mask_shares: Optional[Sequence[int]] = None):
        """Gen (Fig. 14): keys for input mask `r_in` and one output mask per
        interval.  `seeds` (two 128-bit DCF root seeds) and `mask_shares`
        (party 0's share z_0 of every interval) replace the CSPRNG for
        reproducible fixtures; give both or neither."""
        if (seeds is None) != (mask_shares is None):
            raise ValueError("seeds and mask_shares must be given together")
        if mask_shares is not None and len(mask_shares) != self.num_intervals:
            raise ValueError("one mask share per interval")
        rw, rp = _words_ptr(r_out, len(r_out))
        sw = u128_words(list(seeds)) if seeds is not None else None
        zw = None
        if mask_shares is not None:
            zw, _ = _words_ptr(mask_shares, len(mask_shares))
        k0 = ctypes.POINTER(ctypes.c_uint8)()
        k1 = ctypes.POINTER(ctypes.c_uint8)()
        n0, n1 = ctypes.c_size_t(), ctypes.c_size_t()
        check(_lib.lib().dpf_amd_mic_gen(
            self._h, r_in & MASK64, (r_in >> 64) & MASK64, rp, len(r_out),
            sw.ctypes.data_as(ctypes.c_void_p) if sw is not None else None,
            zw.ctypes.data_as(ctypes.c_void_p) if zw is not None else None,
            ctypes.byref(k0), ctypes.byref(n0), ctypes.byref(k1), ctypes.byref(n1)))
        return MicKey(take_buffer(k0, n0)), MicKey(take_buffer(k1, n1))

    def batch_eval(self, keys: Sequence[MicKey], evaluation_points) -> List[int]:
        """BatchEval: keys[i] at evaluation_points[i]; the share of key i and
        interval j is at i * num_intervals + j."""
        datas = [bytes(k) for k in keys]
        arr = (ctypes.c_char_p * max(len(datas), 1))(*datas)
        lens = (ctypes.c_size_t * max(len(datas), 1))(*[len(d) for d in datas])
        npts = len(evaluation_points)
        pw, pp = _words_ptr(evaluation_points, npts)
        count = len(keys) * self.num_intervals
        out = np.zeros((max(count, 1), 2), dtype=np.uint64)
        check(_lib.lib().dpf_amd_mic_batch_eval(
            self._h, arr, lens, len(keys), pp, npts, out.ctypes.data_as(ctypes.c_void_p)))
        return [int(lo) | (int(hi) << 64) for lo, hi in out[:count].tolist()]

    def eval(self, key: MicKey, x: int) -> List[int]:
        """Eval(k, x): one share per interval."""
        return self.batch_eval([key], [x])
