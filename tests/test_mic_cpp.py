"""The reference's MultipleIntervalContainmentGate C++ API as a drop-in
(tests/cpp/mic_api_test.cc): a plain g++ program written against
include/dpf_amd/multiple_interval_containment.h and linked to libdpf_amd.so
- ports of GenAndEvalSucceedsForSmallGroup, GenAndEvalSucceedsForLargeGroup
and BatchEvalIsSameAsRepeatedEval (multiple_interval_containment_test.cc).
Built by build_native; it runs on the GPU and exits 0."""
import os
import subprocess

import pytest

from distributed_point_functions_amd import build_native


@pytest.mark.gpu
def test_mic_api_program_runs(cuda):
    assert os.path.exists(build_native.MIC_TEST), "run build_native first"
    r = subprocess.run([build_native.MIC_TEST], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "all checks passed" in r.stdout
