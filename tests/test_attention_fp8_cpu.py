"""FP8 attention without a GPU: the binding facts of the two entry points and the wrappers' refusal of CPU tensors."""
from pathlib import Path

import pytest
import torch


@pytest.mark.parametrize("name", ["da_attention_fp8_prepare", "da_attention_fp8"])
def test_lib_facts(name):
    from diffusers_amd import _lib as L
    assert name in L.SIGNATURES and name in L.PASS_THROUGH and L.PASS_THROUGH[name].endswith("refuses under a recording")
    assert name not in L.FN_IDS and name not in L.NOT_PLANNABLE and list(L.PASS_THROUGH)[-1] != name
    assert L.ABI_VERSION == 9 and L.FN_COUNT == 36
    header = (Path(__file__).resolve().parent.parent / "include" / "diffusers_amd.h").read_text()
    assert f"int {name}(" in header and "} da_attention_fp8_params;" in header


def test_ops_refuse_cpu_tensors():
    from diffusers_amd import ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.attention_fp8_prepare(torch.zeros((8, 256), dtype=torch.bfloat16), torch.zeros((128, 8), dtype=torch.bfloat16), B=1, S=8, H=1)
    q, s = torch.zeros((8, 128), dtype=torch.float8_e4m3fn), torch.ones((8, 1))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.attention_fp8(q, q, torch.zeros((128, 128), dtype=torch.float8_e4m3fn), s, s, torch.ones((1, 128)), B=1, H=1, Sq=8, Skv=8,
                          scale=1.0)
