#!/usr/bin/env python
"""Writes tests/golden/scheduler_paths.npz and scheduler_paths.json: every case of tests/scheduler_paths.py run once on the CPU over
the logging stand-ins of the sampler kernels, plus this host's fp32 libm probe (scheduler_paths.libm_probe).
tests/test_scheduler_paths_cpu.py compares later runs with these files -- bit for bit on a host whose probe is the recorded one -- so
they are recorded BEFORE a change of diffusers_amd/schedulers.py and committed unchanged with it.  ``--check`` is always bitwise.

    python tools/record_scheduler_paths.py            # rewrite the golden files
    python tools/record_scheduler_paths.py --check    # run the table, report what differs, write nothing
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import scheduler_paths as SP  # noqa: E402

GOLDEN = ROOT / "tests" / "golden"


def run_table():
    arrays, errors = {}, {}
    with pytest.MonkeyPatch.context() as mp:
        SP.install(mp)
        for name in SP.CASES:
            a, meta = SP.record(name)
            arrays.update({f"{name}:{k}": v for k, v in a.items()})
            arrays[f"{name}:meta"] = np.array(json.dumps(meta, sort_keys=True))
        for name in SP.ERRORS:
            errors[name] = SP.record_error(name)
    arrays.update({f"{SP.PROBE}:{k}": v for k, v in SP.libm_probe().items()})
    return arrays, errors


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--check", action="store_true", help="compare with the golden files instead of writing them")
    args = ap.parse_args()
    arrays, errors = run_table()
    unrefused = [k for k, v in errors.items() if v["type"] is None]
    if unrefused and not args.check:
        sys.exit(f"these error cases raise nothing: {unrefused}")
    if args.check:
        with np.load(GOLDEN / "scheduler_paths.npz") as z:
            gold = {k: z[k] for k in z.files}
        gold_err = json.loads((GOLDEN / "scheduler_paths.json").read_text())
        bad = sorted(k for k in set(gold) | set(arrays)
                     if k not in gold or k not in arrays or gold[k].dtype != arrays[k].dtype
                     or gold[k].tobytes() != arrays[k].tobytes())
        bad += sorted(k for k in set(gold_err) | set(errors) if gold_err.get(k) != errors.get(k))
        cases = sorted({k.split(":")[0] for k in bad})
        print(f"{len(cases)} of {len(SP.CASES) + len(SP.ERRORS)} cases differ" + "".join(f"\n  {c}" for c in cases))
        sys.exit(1 if bad else 0)
    np.savez_compressed(GOLDEN / "scheduler_paths.npz", **arrays)
    (GOLDEN / "scheduler_paths.json").write_text(json.dumps(errors, indent=1, sort_keys=True) + "\n")
    print(f"{len(SP.CASES)} cases, {len(SP.ERRORS)} refusals -> {GOLDEN / 'scheduler_paths.npz'} "
          f"({(GOLDEN / 'scheduler_paths.npz').stat().st_size} bytes)")


if __name__ == "__main__":
    main()
