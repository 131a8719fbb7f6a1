"""MotionAdapter.from_pretrained on the CPU: a reference-layout checkpoint (with the ``pos_embed.pe`` buffers real checkpoints carry) packs
once, and the second load comes from the pack-once cache with the same tensors."""
import torch

from diffusers_amd import MotionAdapter, init as dinit, packed_cache
from diffusers_amd.loading import LazyCheckpoint, save_reference_checkpoint
from diffusers_amd.motion_adapter import motion_adapter_param_shapes, sinusoidal_pe


def test_from_pretrained_packs_once_and_ignores_the_pe_buffer(tmp_path, monkeypatch):
    cfg = dict(MotionAdapter.DEFAULTS, block_out_channels=(320,), motion_layers_per_block=1)
    sd = dinit.random_state_dict(motion_adapter_param_shapes(cfg), seed=2)
    sd.update({k[:-len("norm1.weight")] + "pos_embed.pe": sinusoidal_pe(320)[None] for k in list(sd) if k.endswith("norm1.weight")})
    d = save_reference_checkpoint(sd, dict(cfg, _class_name="MotionAdapter"), tmp_path / "adapter")
    first = MotionAdapter.from_pretrained(d, device="cpu")
    assert len(list((d / "diffusers_amd_packed").glob("MotionAdapter-*.safetensors"))) == 1
    assert [len(b) for b in first.down] == [1] and [len(b) for b in first.up] == [2] and len(first.mid) == 1
    monkeypatch.setattr(LazyCheckpoint, "__getitem__", lambda self, key: 1 / 0)      # the second load reads no checkpoint tensor
    again = MotionAdapter.from_pretrained(d, device="cpu")
    a, b = packed_cache.packed_tensors(first), packed_cache.packed_tensors(again)
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    same = MotionAdapter.from_state_dict({k: v for k, v in sd.items() if not k.endswith(".pe")}, device="cpu", **cfg)
    assert all(torch.equal(t, u) for t, u in zip(a.values(), packed_cache.packed_tensors(same).values()))
