"""Timing of the tiled AutoencoderKL.encode (seeded random weights and images: timings only), every comparison with both legs in one
process on one GPU, alternating, median of the repetitions with min .. max:

  (a) blend and place  the nine ops.vae_moments_tile_blend launches of one SDXL-default tiled encode of a 2048 x 2048 image (tiles of
                       1024 px = 128 latent, blend extent 32, 3 x 3 tiles, 8 x 256 x 256 moments) on synthetic conv_out results,
                       against the same work as the reference does it, with torch ops on the GPU: the 1 x 1 quant_conv of each tile,
                       blend_extent row / column operations per seam, the crops, a torch.cat per row and one of the rows
  (b) encode           AutoencoderKL.encode_image (the SDXL VAE, an fp32 NCHW image, normalize=True) tiled against untiled at the
                       given image sizes: time and the peak of torch.cuda.max_memory_allocated above what is allocated before the
                       call.  An untiled leg that runs out of memory is recorded as such, once, and not tried again

One part (and, for (b), one size) per invocation keeps every GPU step a process of its own that a caller can put under a time limit:

    timeout -k 10 300 python tools/bench_vae_tiled_encode.py --part a
    timeout -k 10 300 python tools/bench_vae_tiled_encode.py --part b --sizes 1024
    timeout -k 10 600 python tools/bench_vae_tiled_encode.py --part b --sizes 2048
    timeout -k 10 900 python tools/bench_vae_tiled_encode.py --part b --sizes 4096

Prints one JSON line; --markdown PATH also writes that part's table.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
bf16 = torch.bfloat16


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _stats(v):
    v = sorted(v)
    return {"median_ms": round(v[len(v) // 2], 3), "min_ms": round(v[0], 3), "max_ms": round(v[-1], 3)}


def _alternate(legs: dict, reps: int, warm: int = 2) -> dict:
    for fn in legs.values():
        for _ in range(warm):
            fn()
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            times[k].append(_timed(fn))
    return {k: _stats(v) for k, v in times.items()}


def blend_and_place(reps: int) -> dict:
    from diffusers_amd import init as dinit, ops
    from diffusers_amd.autoencoder_kl import AutoencoderKL
    dev = torch.device("cuda", 0)
    vae = AutoencoderKL(**dinit.SDXL_VAE)                      # host bookkeeping only: no weights
    E, rows, HL, WL = vae._encode_tile_plan(2048, 2048)
    row_limit = vae.tile_latent_min_size - E
    g = torch.Generator().manual_seed(0)
    wq = (torch.randn(8, 8, generator=g) * 0.5).to(bf16).to(dev)
    bq = (torch.randn(8, generator=g) * 0.1).to(bf16).to(dev)
    raw, nchw = [], []
    for row in rows:
        raw.append([]), nchw.append([])
        for t in row:
            x = torch.randn(1, t["h"] * t["w"], 16, generator=g).to(bf16).to(dev)          # the implicit-GEMM conv_out's result
            raw[-1].append((x, (t["h"] * t["w"] * 16, 1, 16)))
            nchw[-1].append(x[:, :, :8].permute(0, 2, 1).reshape(1, 8, t["h"], t["w"]).contiguous())
    moments = torch.empty((1, 8, HL, WL), device=dev, dtype=bf16)

    def fused():
        above = None
        for r, row in enumerate(rows):
            done = []
            for c, t in enumerate(row):
                x, st = raw[r][c]
                done.append(ops.vae_moments_tile_blend(x, st, batch=1, latent_channels=4, height=t["h"], width=t["w"], moments=moments,
                                                       y0=t["y0"], x0=t["x0"], keep_h=t["keep_h"], keep_w=t["keep_w"], wq=wq, bq=bq,
                                                       extent=E, up=above[c] if above is not None else None,
                                                       left=done[-1] if done else None,
                                                       want_fin=r + 1 < len(rows) or c + 1 < len(row)))
            above = done
        return moments

    w4 = wq.view(8, 8, 1, 1)

    def torch_ops():
        tiles = [[F.conv2d(t, w4, bq) for t in row] for row in nchw]                        # quant_conv(encoder(tile))
        out_rows = []
        for i, row in enumerate(tiles):
            out = []
            for j, b in enumerate(row):
                if i > 0:
                    a = tiles[i - 1][j]
                    for y in range(min(a.shape[2], b.shape[2], E)):
                        b[:, :, y, :] = a[:, :, -E + y, :] * (1 - y / E) + b[:, :, y, :] * (y / E)
                if j > 0:
                    a = row[j - 1]
                    for x in range(min(a.shape[3], b.shape[3], E)):
                        b[:, :, :, x] = a[:, :, :, -E + x] * (1 - x / E) + b[:, :, :, x] * (x / E)
                out.append(b[:, :, :row_limit, :row_limit])
            out_rows.append(torch.cat(out, dim=3))
        return torch.cat(out_rows, dim=2)

    a, b = fused().float(), torch_ops().float()
    res = _alternate({"fused": fused, "torch_ops": torch_ops}, reps)
    res.update(tiles=[len(rows), len(rows[0])], blend_extent=E, moments=[HL, WL], launches_fused=sum(len(r) for r in rows),
               outputs_equal=bool(torch.equal(a, b)), max_abs_diff=float((a - b).abs().max()),
               torch_over_fused=round(res["torch_ops"]["median_ms"] / res["fused"]["median_ms"], 1))
    return res


def encodes(reps: int, sizes) -> dict:
    from diffusers_amd import factory, init as dinit
    dev = torch.device("cuda", 0)
    vae, _ = factory.build_vae(dinit.SDXL_VAE, seed=1, device=dev, init_device=str(dev), with_encoder=True)
    out = {}
    for px in sizes:
        img = torch.rand(1, 3, px, px, generator=torch.Generator().manual_seed(px)).to(dev)
        legs = {"untiled": False, "tiled": True}
        times, peak, failed = {k: [] for k in legs}, {k: 0 for k in legs}, {}

        def run(k):
            vae.use_tiling = legs[k]
            return vae.encode_image(img, nchw=True, normalize=True).parameters

        for k in list(legs):
            try:
                for _ in range(2):
                    run(k)
            except torch.cuda.OutOfMemoryError as e:            # recorded once, the leg is not tried again
                failed[k] = "out of memory: " + str(e).split("\n")[0][:160]
                del legs[k]
                torch.cuda.empty_cache()
        for _ in range(reps):
            for k in legs:
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                times[k].append(_timed(lambda: run(k)))
                peak[k] = max(peak[k], torch.cuda.max_memory_allocated() - base)
        vae.use_tiling = False
        res = {k: dict(_stats(times[k]), peak_mib=round(peak[k] / 2 ** 20, 1)) for k in legs}
        res.update({k: {"failed": why} for k, why in failed.items()})
        res["tiles"] = sum(len(r) for r in vae._encode_tile_plan(px, px)[1]) if px > vae.tile_sample_min_size else 1
        out[str(px)] = res
        torch.cuda.empty_cache()
    return out


def markdown(out: dict) -> str:
    lines = [f"`tools/bench_vae_tiled_encode.py`, {out['device']}, legs alternating in one process, median of {out['reps']} (min .. max).", ""]
    if "blend_and_place" in out:
        a = out["blend_and_place"]
        lines += ["### (a) Blend and place: one SDXL-default tiled encode of a 2048 x 2048 image", "",
                  f"{a['tiles'][0]} x {a['tiles'][1]} tiles, blend extent {a['blend_extent']}, moments 8 x {a['moments'][0]} x {a['moments'][1]}; "
                  f"outputs equal to the bit: {a['outputs_equal']} (max abs difference {a['max_abs_diff']}).", "",
                  "| leg | median ms | min | max |", "|---|---|---|---|"]
        for k, name in (("fused", f"`da_vae_moments_tile_blend`, {a['launches_fused']} launches"),
                        ("torch_ops", "torch ops (quant_conv, row / column blends, crops, cats)")):
            lines.append(f"| {name} | {a[k]['median_ms']} | {a[k]['min_ms']} | {a[k]['max_ms']} |")
        lines += ["", f"torch ops / fused = {a['torch_over_fused']} x.", ""]
    if "encode" in out:
        lines += ["### (b) encode_image, SDXL VAE, fp32 NCHW image, batch 1", "",
                  "| image | leg | tiles | median ms | min | max | peak MiB above the call's start |", "|---|---|---|---|---|---|---|"]
        for px, res in out["encode"].items():
            for k in ("untiled", "tiled"):
                tiles = 1 if k == "untiled" else res["tiles"]
                if "failed" in res[k]:
                    lines.append(f"| {px} x {px} | {k} | {tiles} | {res[k]['failed']} | | | |")
                else:
                    lines.append(f"| {px} x {px} | {k} | {tiles} | {res[k]['median_ms']} | {res[k]['min_ms']} | {res[k]['max_ms']} | {res[k]['peak_mib']} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("a", "b", "ab"), default="ab")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1024,2048,4096")
    ap.add_argument("--markdown", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vae_tiled_encode: no HIP device (timings are taken on the GPU only)")
    out = {"tool": "bench_vae_tiled_encode", "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    if "a" in args.part:
        out["blend_and_place"] = blend_and_place(args.reps)
    if "b" in args.part:
        out["encode"] = encodes(args.reps, [int(s) for s in args.sizes.split(",")])
    if args.markdown:
        Path(args.markdown).write_text(markdown(out))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
