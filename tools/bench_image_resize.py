"""Timing of the image resize (seeded random bytes: timings only): ops.resample_u8 on the GPU against PIL.Image.resize on the host, RGB,
LANCZOS, for a 4032 x 3024 photo -> 1024 x 768 and a 512 x 512 image -> 1024 x 1024.  Legs alternate in one process; median of the
repetitions with min .. max.  The GPU leg is timed twice: the kernel alone on a resident image (`--inner` back-to-back calls between
two synchronisations, over their number) and the whole of what a pipeline call pays (host array -> device, kernel, synchronise).
The results are compared to the bit before anything is timed.

    python tools/bench_image_resize.py [--reps 5] [--inner 20] [--markdown profiles/image_resize_numbers.md]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
SHAPES = [((3024, 4032), (768, 1024)), ((512, 512), (1024, 1024))]           # (height, width) -> (height, width)


def _stats(v):
    v = sorted(v)
    return {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}


def _timed(fn, inner=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def legs(reps: int, inner: int) -> list:
    from diffusers_amd import ops
    dev, rows = torch.device("cuda", 0), []
    for (hi, wi), (ho, wo) in SHAPES:
        a = np.random.default_rng(hi).integers(0, 256, size=(hi, wi, 3), dtype=np.uint8)
        photo, host, resident = Image.fromarray(a), torch.from_numpy(a)[None], torch.from_numpy(a)[None].to(dev)
        want = torch.from_numpy(np.asarray(photo.resize((wo, ho), Image.LANCZOS)))
        if not torch.equal(ops.resample_u8(resident, (ho, wo), "lanczos")[0].cpu(), want):
            raise SystemExit(f"bench_image_resize: {hi} x {wi} -> {ho} x {wo} differs from Pillow")
        run = {"pillow_host": (lambda: photo.resize((wo, ho), Image.LANCZOS), 1),
               "kernel": (lambda: ops.resample_u8(resident, (ho, wo), "lanczos"), inner),
               "upload_and_kernel": (lambda: ops.resample_u8(host.to(dev), (ho, wo), "lanczos"), 1)}
        for fn, _ in run.values():
            fn(), fn()
        times = {k: [] for k in run}
        for _ in range(reps):
            for k, (fn, n) in run.items():
                times[k].append(_timed(fn, n))
        route, tile, _ = ops.resample_route(1, (hi, wi), (ho, wo), 3, "lanczos")
        res = {k: _stats(v) for k, v in times.items()}
        res.update(src=[hi, wi], dst=[ho, wo], route=route, tile=list(tile),
                   pillow_over_kernel=round(res["pillow_host"]["median_ms"] / res["kernel"]["median_ms"], 1),
                   pillow_over_upload_and_kernel=round(res["pillow_host"]["median_ms"] / res["upload_and_kernel"]["median_ms"], 1))
        rows.append(res)
    return rows


def markdown(out: dict) -> str:
    fmt = lambda r: f"{r['median_ms']} ({r['min_ms']} .. {r['max_ms']})"  # noqa: E731
    lines = ["# Image resize: measurements", "", f"`tools/bench_image_resize.py`, {out['device']} against Pillow {out['pillow']} on the host, RGB, "
             f"LANCZOS; legs alternating in one process, median of {out['reps']} (min .. max), ms.  `kernel`: the image resident on the "
             f"device, {out['inner']} back-to-back calls over their number; `upload + kernel`: host array -> device, kernel, synchronise "
             "(what a pipeline call pays).  Results equal Pillow's to the bit (checked before timing).  Reported, not gated.", "",
             "| height x width | route, tile | Pillow (host) | kernel | upload + kernel | Pillow / kernel | Pillow / (upload + kernel) |",
             "|---|---|---|---|---|---|---|"]
    for r in out["rows"]:
        lines.append(f"| {r['src'][0]} x {r['src'][1]} -> {r['dst'][0]} x {r['dst'][1]} | {r['route']}, {r['tile'][0]} x {r['tile'][1]} | "
                     f"{fmt(r['pillow_host'])} | {fmt(r['kernel'])} | {fmt(r['upload_and_kernel'])} | {r['pillow_over_kernel']} x | "
                     f"{r['pillow_over_upload_and_kernel']} x |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--markdown", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_image_resize: no HIP device (timings are taken on the GPU only)")
    import PIL
    out = {"tool": "bench_image_resize", "reps": args.reps, "inner": args.inner, "device": torch.cuda.get_device_name(0),
           "pillow": PIL.__version__, "rows": legs(args.reps, args.inner)}
    if args.markdown:
        Path(args.markdown).write_text(markdown(out))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
