"""FP8 linears without a GPU: the binding facts of the two entry points and the wrappers' refusal of CPU tensors."""
from pathlib import Path

import pytest
import torch

NAMES = ("da_quantize_rows_e4m3", "da_gemm_fp8")


@pytest.mark.parametrize("name", NAMES)
def test_lib_facts(name):
    from diffusers_amd import _lib as L
    assert name in L.SIGNATURES and name in L.PASS_THROUGH and "refuses under a recording" in L.PASS_THROUGH[name]
    assert name not in L.FN_IDS and name not in L.NOT_PLANNABLE and list(L.PASS_THROUGH)[-1] != name and L.ABI_VERSION == 9
    header = (Path(__file__).resolve().parent.parent / "include" / "diffusers_amd.h").read_text()
    assert f"int {name}(" in header


def test_ops_refuse_cpu_tensors():
    from diffusers_amd import ops
    q, s = torch.zeros((16, 128), dtype=torch.float8_e4m3fn), torch.ones(16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.quantize_rows_fp8(torch.zeros((16, 128), dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.linear_fp8(q, s, q, s)
