"""Generates tests/golden/mic/mic.json: MIC gate wire fixtures serialized by
the google.protobuf runtime (tests/mic_wire_schema.py) rather than by the
project's codecs.

Per case: MicParameters bytes, and the two MicKey messages Fig. 14 Gen makes
for the recorded input mask, output masks, DCF root seeds and party-0 mask
shares - the DcfKey from the oracle's incremental keys (oracle/dpf_oracle.c)
for alpha = (N - 1 + r_in) mod N, beta = 1, the mask shares from line 5 of
Gen restated here.

Run from the repo root:
    python tests/golden/mic/make_mic.py
"""
from __future__ import annotations

import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

from oracle import pyoracle as po  # noqa: E402
from tests import mic_wire_schema as MW  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location(
    "make_wire", os.path.join(os.path.dirname(HERE), "wire", "make_wire.py"))
make_wire = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make_wire)

SPEC = ("int", 128)

# name, log_group_size, intervals, r_in, r_out, seeds, z_0
CASES = [
    ("log1", 1, [(0, 0), (0, 1), (1, 1)], 1, [1, 0, 1], (11, 12), [1, 0, 1]),
    ("log10", 10, [(0, 0), (5, 900), (1023, 1023), (0, 1023)], 1000, [3, 0, 1023, 512],
     (0x1234, 0x5678), [7, 1023, 0, 99]),
    ("log64", 64, [(10, 45), (23, 30), (15, 15)], (1 << 64) - 7, [1 << 63, 5, 0],
     (1 << 100, (1 << 127) + 3), [(1 << 64) - 1, 0, 12345678901234567890]),
    ("log127", 127, [(1 << 126, (1 << 126) + 3), ((1 << 127) - 1, (1 << 127) - 1)],
     (1 << 126) + 12345, [(1 << 127) - 1, 1 << 100], (5, 6), [1 << 126, (1 << 127) - 2]),
]


def line5(N, p, q, r_in, r_out):
    """z of Fig. 14 Gen line 5 (multiple_interval_containment.cc:166-180)."""
    q_prime = (q + 1) % N
    alpha_p, alpha_q, alpha_q_prime = (p + r_in) % N, (q + r_in) % N, (q + 1 + r_in) % N
    return (r_out + (alpha_p > alpha_q) - (alpha_p > p) + (alpha_q_prime > q_prime)
            + (alpha_q == N - 1)) % N


def main():
    out = {}
    for name, n, intervals, r_in, r_out, seeds, z0 in CASES:
        N = 1 << n
        levels = [(i, SPEC, 0) for i in range(n)]
        od = po.Dpf(levels)
        gamma = (N - 1 + r_in) % N
        betas = [1 if (gamma >> (n - 1 - i)) & 1 else 0 for i in range(n)]
        oracle_keys = od.generate_keys(gamma >> 1, betas, seeds=seeds)
        keys = []
        for party, ok in enumerate(oracle_keys):
            k = MW.cls("MicKey")()
            k.dcfkey.key.CopyFrom(make_wire.key_message(od, levels, ok))
            for (p, q), r, z_0 in zip(intervals, r_out, z0):
                z = line5(N, p, q, r_in, r)
                MW.set_uint128(k.output_mask_share.add(), z_0 % N if party == 0
                               else (z - z_0) % N)
            keys.append(make_wire.ser(k).hex())
        out[name] = {
            "log_group_size": n,
            "intervals": [[str(p), str(q)] for p, q in intervals],
            "r_in": str(r_in), "r_out": [str(r) for r in r_out],
            "seeds": [str(s) for s in seeds], "z0": [str(z) for z in z0],
            "parameters": make_wire.ser(MW.parameters(n, intervals)).hex(),
            "keys": keys,
        }
    with open(os.path.join(HERE, "mic.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", len(out), "cases")


if __name__ == "__main__":
    main()
