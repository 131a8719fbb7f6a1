"""Timing of the tiled AutoencoderKL.decode (seeded random weights and tiles: timings only), every comparison with both legs in one
process on one GPU, alternating, median of the repetitions with min .. max:

  (a) blend and place  the nine ops.vae_tile_blend launches of one SDXL-default tiled decode of 256 x 256 latents (tiles of 1024 px,
                       blend extent 256, 3 x 3 tiles, a 2048 x 2048 uint8 image) on synthetic conv_out results, against the same
                       work as the reference does it, with torch ops on the GPU: blend_extent row / column operations per seam,
                       the crops, a torch.cat per row and one of the rows, and the image processor's postprocess over the full image
  (b) decode           AutoencoderKL.decode (the SDXL VAE, postprocess="uint8") tiled against untiled at 128 x 128, 256 x 256 and
                       512 x 512 latents: time and the peak of torch.cuda.max_memory_allocated above what is allocated before the
                       call.  At 128 x 128 the default tile (128 latents) does not tile at all, so that size is also run with the
                       SD VAE's tile (tile_sample_min_size 512, tile_latent_min_size 64)

Prints one JSON line; --markdown PATH also writes the tables.

    python tools/bench_vae_tiling.py [--reps 5] [--sizes 128,256,512] [--markdown profiles/vae_tiling_numbers.md]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

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
    E, rows, IH, IW = vae._tile_plan(256, 256)
    row_limit = vae.tile_sample_min_size - E
    g = torch.Generator().manual_seed(0)
    raw, nchw = [], []
    for row in rows:
        raw.append([]), nchw.append([])
        for t in row:
            x = torch.randn(1, t["h"] * t["w"], 16, generator=g).to(bf16).to(dev)          # the implicit-GEMM conv_out's result
            raw[-1].append((x, (t["h"] * t["w"] * 16, 1, 16)))
            nchw[-1].append(x[:, :, :3].permute(0, 2, 1).reshape(1, 3, t["h"], t["w"]).contiguous())
    image = torch.empty((1, IH, IW, 3), device=dev, dtype=torch.uint8)

    def fused():
        above = None
        for r, row in enumerate(rows):
            done = []
            for c, t in enumerate(row):
                x, st = raw[r][c]
                done.append(ops.vae_tile_blend(x, st, batch=1, channels=3, height=t["h"], width=t["w"], image=image, y0=t["y0"],
                                               x0=t["x0"], keep_h=t["keep_h"], keep_w=t["keep_w"], postprocess="uint8", extent=E,
                                               up=above[c] if above is not None else None, left=done[-1] if done else None,
                                               want_fin=r + 1 < len(rows) or c + 1 < len(row)))
            above = done
        return image

    def torch_ops():
        tiles = [[t.clone() for t in row] for row in nchw]     # the reference blends in place on the decoded tiles: fresh ones per pass
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
        img = torch.cat(out_rows, dim=2)
        img = (img.float() * 0.5 + 0.5).clamp(0, 1)            # VaeImageProcessor.postprocess, output_type="pil" up to the PIL call
        return (img.permute(0, 2, 3, 1) * 255).round().to(torch.uint8)

    same = bool(torch.equal(fused(), torch_ops()))
    res = _alternate({"fused": fused, "torch_ops": torch_ops}, reps)
    res.update(tiles=[len(rows), len(rows[0])], blend_extent=E, image=[IH, IW], launches_fused=sum(len(r) for r in rows),
               outputs_equal=same, torch_over_fused=round(res["torch_ops"]["median_ms"] / res["fused"]["median_ms"], 1))
    return res


def decodes(reps: int, sizes) -> dict:
    from diffusers_amd import factory, init as dinit
    dev = torch.device("cuda", 0)
    vae, _ = factory.build_vae(dinit.SDXL_VAE, seed=1, device=dev, init_device=str(dev))
    out = {}
    for lat in sizes:
        z = torch.randn(1, 4, lat, lat, generator=torch.Generator().manual_seed(lat)).to(bf16).to(dev)
        legs = {"untiled": (False, 1024, 128), "tiled": (True, 1024, 128)}
        if lat <= 128:
            legs["tiled_512px_tile"] = (True, 512, 64)
        times, peak = {k: [] for k in legs}, {k: 0 for k in legs}

        def run(k):
            vae.use_tiling, vae.tile_sample_min_size, vae.tile_latent_min_size = legs[k]
            return vae.decode(z, latents_div=0.13025, postprocess="uint8").sample

        for k in legs:
            for _ in range(2):
                run(k)
        for _ in range(reps):
            for k in legs:
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                times[k].append(_timed(lambda: run(k)))
                peak[k] = max(peak[k], torch.cuda.max_memory_allocated() - base)
        vae.use_tiling, vae.tile_sample_min_size, vae.tile_latent_min_size = False, 1024, 128
        res = {k: dict(_stats(times[k]), peak_mib=round(peak[k] / 2 ** 20, 1)) for k in legs}
        res["tiles"] = len(vae._tile_plan(lat, lat)[1]) ** 2 if lat > 128 else 1
        out[str(lat)] = res
        torch.cuda.empty_cache()
    return out


def markdown(out: dict) -> str:
    a, lines = out["blend_and_place"], []
    lines += ["# Tiled AutoencoderKL.decode: measurements", "",
              f"`tools/bench_vae_tiling.py`, {out['device']}, legs alternating in one process, median of {out['reps']} (min .. max).", "",
              "## (a) Blend and place: one SDXL-default tiled decode of 256 x 256 latents", "",
              f"{a['tiles'][0]} x {a['tiles'][1]} tiles, blend extent {a['blend_extent']}, image {a['image'][0]} x {a['image'][1]} uint8; "
              f"outputs equal to the bit: {a['outputs_equal']}.", "",
              "| leg | median ms | min | max |", "|---|---|---|---|"]
    for k, name in (("fused", f"`da_vae_tile_blend`, {a['launches_fused']} launches"), ("torch_ops", "torch ops (row / column blends, cats, postprocess)")):
        lines.append(f"| {name} | {a[k]['median_ms']} | {a[k]['min_ms']} | {a[k]['max_ms']} |")
    lines += ["", f"torch ops / fused = {a['torch_over_fused']} x.  The torch leg blends in place, so each timed pass first clones the nine decoded "
              "tiles (54 MB of copies, not timed separately); both legs are timed from the host around one pass.", "", "## (b) Decode, SDXL VAE, postprocess=\"uint8\", batch 1", "",
              "| latents | leg | tiles | median ms | min | max | peak MiB above the call's start |", "|---|---|---|---|---|---|---|"]
    for lat, res in out["decode"].items():
        for k in ("untiled", "tiled", "tiled_512px_tile"):
            if k in res:
                tiles = 1 if k == "untiled" else res["tiles"] if k == "tiled" else "SD tile (512 px)"
                lines.append(f"| {lat} x {lat} | {k} | {tiles} | {res[k]['median_ms']} | {res[k]['min_ms']} | {res[k]['max_ms']} | {res[k]['peak_mib']} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="128,256,512")
    ap.add_argument("--markdown", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vae_tiling: no HIP device (timings are taken on the GPU only)")
    out = {"tool": "bench_vae_tiling", "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "blend_and_place": blend_and_place(args.reps), "decode": decodes(args.reps, [int(s) for s in args.sizes.split(",")])}
    if args.markdown:
        Path(args.markdown).write_text(markdown(out))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
