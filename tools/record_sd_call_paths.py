#!/usr/bin/env python
"""Writes tests/golden/sd_call_paths.npz and sd_call_paths.json: every case of tests/sd_call_paths.py run once on the CPU
stand-ins of the kernels.  tests/test_sd_call_paths_cpu.py compares later runs with these files bit for bit, so they are recorded
BEFORE a change of the SD / SDXL ``__call__`` paths (diffusers_amd/pipelines.py) and committed unchanged with it.

    python tools/record_sd_call_paths.py            # rewrite the golden files
    python tools/record_sd_call_paths.py --check    # run the table, report what differs, write nothing
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

import inpaint_emulation  # noqa: E402
import ops_emulation  # noqa: E402
import sd_call_paths as S  # noqa: E402
from diffusers_amd import ops  # noqa: E402

GOLDEN = ROOT / "tests" / "golden"


def run_table():
    arrays, errors = {}, {}
    with pytest.MonkeyPatch.context() as mp:
        ops_emulation.install(mp, ops)
        inpaint_emulation.install(mp, ops)
        mp.setattr(ops, "TUNING", False)
        for case in S.CASES:
            a, meta = S.record(case)
            arrays.update({f"{case.name}/{k}": v for k, v in a.items()})
            arrays[f"{case.name}/meta"] = np.array(json.dumps(meta, sort_keys=True))
        for case in S.ERRORS:
            errors[case.name] = S.record_error(case)
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
        with np.load(GOLDEN / "sd_call_paths.npz") as z:
            gold = {k: z[k] for k in z.files}
        gold_err = json.loads((GOLDEN / "sd_call_paths.json").read_text())
        bad = sorted(k for k in set(gold) | set(arrays)
                     if k not in gold or k not in arrays or gold[k].dtype != arrays[k].dtype or not np.array_equal(gold[k], arrays[k]))
        bad += sorted(k for k in set(gold_err) | set(errors) if gold_err.get(k) != errors.get(k))
        cases = sorted({k.split("/")[0] for k in bad})
        print(f"{len(cases)} of {len(S.CASES) + len(S.ERRORS)} cases differ" + "".join(f"\n  {c}" for c in cases))
        sys.exit(1 if bad else 0)
    np.savez_compressed(GOLDEN / "sd_call_paths.npz", **arrays)
    (GOLDEN / "sd_call_paths.json").write_text(json.dumps(errors, indent=1, sort_keys=True) + "\n")
    print(f"{len(S.CASES)} calls, {len(S.ERRORS)} refused calls -> {GOLDEN / 'sd_call_paths.npz'} "
          f"({(GOLDEN / 'sd_call_paths.npz').stat().st_size} bytes)")


if __name__ == "__main__":
    main()
