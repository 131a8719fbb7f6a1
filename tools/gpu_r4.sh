#!/bin/bash
# Round-4 gpurun stages.  usage: gpu_r4.sh "attn attntest ..."
R=${GRAFT_REPO_ROOT:-/root/repo}
O=$R/gpurun_out
mkdir -p $O
cd $R
WHAT=${1:-attn}
if [[ $WHAT == *attntest* ]]; then
  timeout 600 python -m pytest tests/test_kernels_gpu.py -m gpu -q -s --timeout 300 -k "attention" > $O/pytest_attn.log 2>&1; echo "pytest attn rc=$?"
  grep -E "passed|failed|FAILED|Error" $O/pytest_attn.log | tail -20
  grep -E "\[parity\] flash attn (v2|spiked)" $O/pytest_attn.log | tail -30
fi
if [[ $WHAT == *attnbench* ]]; then
  rm -f $O/attn_r4.jsonl
  timeout 600 python tools/bench_attn_r4.py $O/attn_r4.jsonl > $O/attn_r4.log 2>&1; echo "attn bench rc=$?"
  tail -3 $O/attn_r4.log | cut -c1-300
fi
if [[ $WHAT == *benchfast* ]]; then
  timeout 900 python bench.py --full --steps 3 --warmup 1 --no-reference --no-cpu-baseline > $O/bench.json 2> $O/bench.err; echo "bench rc=$?"
  cut -c1-1200 $O/bench.json; grep "^\[bench" $O/bench.err | tail -20
fi
if [[ $WHAT == *others* ]]; then
  for cfg in flux wan sd15; do
    ST=2; [[ $cfg == wan ]] && ST=1
    timeout 900 python bench.py --full --config $cfg --steps $ST --warmup 1 > $O/bench_$cfg.json 2> $O/bench_$cfg.err; echo "$cfg rc=$?"
    cut -c1-400 $O/bench_$cfg.json; tail -2 $O/bench_$cfg.err | cut -c1-300
  done
fi
if [[ $WHAT == *lnfold* ]]; then
  timeout 600 python -m pytest tests/test_gemm_k2_gpu.py tests/test_kernels_gpu.py -m gpu -q -s --timeout 300 -k "layernorm_fold" > $O/pytest_lnfold.log 2>&1; echo "pytest lnfold rc=$?"
  grep -E "passed|failed|FAILED|Error|assert" $O/pytest_lnfold.log | tail -20
  rm -f $O/lnfold_r4.jsonl
  timeout 300 python tools/bench_lnfold_r4.py $O/lnfold_r4.jsonl > $O/lnfold_r4.log 2>&1; echo "lnfold bench rc=$?"
  cat $O/lnfold_r4.jsonl | cut -c1-600
fi
if [[ $WHAT == *norms* ]]; then
  rm -f $O/norms_r4.jsonl
  timeout 120 python tools/bench_norms_r4.py $O/norms_r4.jsonl > $O/norms_r4.log 2>&1; echo "norms default rc=$?"
  for kn in "DA_GN_THREADS=512" "DA_GN_MINPIX=16" "DA_GN_MINPIX=4" "DA_GN_MAXBLK=1024 DA_GN_CAP=4096" "DA_GN_THREADS=512 DA_GN_MINPIX=16" "DA_GN_MAXBLK=256"; do
    env $kn timeout 120 python tools/bench_norms_r4.py $O/norms_r4.jsonl >> $O/norms_r4.log 2>&1
  done
  grep "sum over\|layernorm" $O/norms_r4.jsonl | cut -c1-200
fi
if [[ $WHAT == *foldab* ]]; then
  for mode in 0 2 1 0 2; do
    DIFFUSERS_AMD_LN_FOLD=$mode timeout 600 python bench.py --steps 3 --warmup 1 --no-reference --no-cpu-baseline --no-roofline > $O/bench_fold$mode.json 2> $O/bench_fold$mode.err; echo "fold mode $mode rc=$? $(cut -c1-140 $O/bench_fold$mode.json | grep -o '"value": [0-9.]*')"
  done
fi
if [[ $WHAT == *normsdef* ]]; then
  rm -f $O/norms_r4b.jsonl
  timeout 120 python tools/bench_norms_r4.py $O/norms_r4b.jsonl > $O/norms_r4b.log 2>&1; echo "norms rc=$?"
  grep "sum over\|layernorm" $O/norms_r4b.jsonl | cut -c1-200
fi
if [[ $WHAT == *traffic* ]]; then
  cd /tmp && export TMPDIR=/tmp
  rm -rf $O/pmc_traffic; mkdir -p $O/pmc_traffic
  DIFFUSERS_AMD_TUNE=0 timeout 300 rocprofv3 --kernel-trace --pmc FETCH_SIZE -f csv -d $O/pmc_traffic/fetch -o sdxl -- python $R/tools/pmc_one_step.py 2 > $O/pmc_traffic/fetch.log 2>&1; echo "pmc fetch rc=$?"
  DIFFUSERS_AMD_TUNE=0 timeout 300 rocprofv3 --kernel-trace --pmc WRITE_SIZE -f csv -d $O/pmc_traffic/write -o sdxl -- python $R/tools/pmc_one_step.py 2 > $O/pmc_traffic/write.log 2>&1; echo "pmc write rc=$?"
  cd $R
  # algorithmic bytes per launch: from this call's bench line if there is one, else from the last committed line
  ALGO=$(python -c "import json;print(json.load(open('$O/bench_full.json'))['roofline']['algorithmic_bytes_per_launch'])" 2>/dev/null || python -c "import json;print(json.load(open('$R/profiles/r04k_bench_line_full.json'))['roofline']['algorithmic_bytes_per_launch'])" 2>/dev/null)
  python tools/pmc_traffic.py $O/pmc_traffic/fetch $O/pmc_traffic/write $O/r04_sdxl_traffic.md $O/sdxl_traffic.json "$ALGO" 140
  cp $O/sdxl_traffic.json $R/profiles/sdxl_traffic.json   # a later `benchfull` stage of this call reads it (roofline.traffic)
  find $O/pmc_traffic -name '*kernel_trace*' -delete
  find $O/pmc_traffic -name '*counter_collection.csv' -size +8M -delete
  tail -4 $O/pmc_traffic/fetch.log | cut -c1-200
fi
if [[ $WHAT == *benchfull* ]]; then
  timeout 1500 python bench.py --full --steps 3 --warmup 1 > $O/bench_full.json 2> $O/bench_full.err; echo "bench full rc=$?"
  cut -c1-300 $O/bench_full.json; grep "^\[bench" $O/bench_full.err | tail -40
fi
if [[ $WHAT == *plantest* ]]; then
  timeout 900 python -m pytest tests/test_plan_gpu.py -m gpu -q -s --timeout 600 > $O/pytest_plan.log 2>&1; echo "pytest plan rc=$?"
  grep -E "passed|failed|FAILED|Error|assert|\[plan\]|differ|launches" $O/pytest_plan.log | tail -30
  timeout 300 python tools/make_plan_demo.py $O/step.daplan > $O/make_plan.log 2>&1; echo "make plan rc=$?"; tail -3 $O/make_plan.log | cut -c1-600
  rm -f $O/step.daplan
fi
if [[ $WHAT == *fulltest* ]]; then
  timeout 2400 python -m pytest tests -m gpu -q -s --timeout 900 > $O/pytest_gpu.log 2>&1; echo "pytest rc=$?" | tee -a $O/pytest_gpu.log
  grep -E "passed|failed|FAILED|Error" $O/pytest_gpu.log | tail -20
  grep -E "\[parity\] (SDXL|FLUX|Wan|SD1.5|full)|\[drop-in\]" $O/pytest_gpu.log | tail -40
fi
if [[ $WHAT == *prof* ]]; then
  cd /tmp && export TMPDIR=/tmp
  rm -rf $O/prof
  timeout 600 rocprofv3 --kernel-trace --stats -f csv -d $O/prof -o sdxl -- python $R/bench.py --steps 1 --warmup 1 --no-cpu-baseline --no-roofline --no-reference --no-other-configs > $O/prof.log 2>&1; echo "prof rc=$?"
  grep '"metric"' $O/prof.log | cut -c1-200
  find $O/prof -name '*kernel_trace*' -size +30M -delete
  cd $R
  python tools/prof_summary.py $(find $O/prof -name '*kernel_stats.csv' | head -1) "r04 sdxl bench (--steps 1 --warmup 1)" > $O/prof_summary.md 2>> $O/prof.log; head -60 $O/prof_summary.md
fi
if [[ $WHAT == *tunemissing* ]]; then
  # shapes the shipped table does not hold yet (this round: the query-blocked VAE attention GEMMs) are tuned live with both kernel
  # families competing, saved, and merged into a copy of the shipped table (gpurun_out/tuned_merged_r4.json)
  rm -f $O/tuned_new_r4.json
  DIFFUSERS_AMD_GEMM_FAMILY=all DIFFUSERS_AMD_TUNE_SAVE=$O/tuned_new_r4.json timeout 700 python bench.py --steps 1 --warmup 1 --no-cpu-baseline --no-roofline --no-reference --no-other-configs > $O/tunemissing.json 2> $O/tunemissing.err; echo "tunemissing rc=$?"
  for cfg in sd15 flux; do
    DIFFUSERS_AMD_GEMM_FAMILY=all DIFFUSERS_AMD_TUNE_DB=$O/tuned_new_r4.json DIFFUSERS_AMD_TUNE_SAVE=$O/tuned_new_r4.json timeout 700 python bench.py --full --config $cfg --steps 1 --warmup 1 --no-cpu-baseline > $O/tunemissing_$cfg.json 2>> $O/tunemissing.err; echo "tunemissing $cfg rc=$?"
  done
  python - <<PYEOF
import json
a = json.load(open("$R/diffusers_amd/tuned/gfx950.json"))
try:
    b = json.load(open("$O/tuned_new_r4.json"))
except Exception as e:
    b = {"entries": {}}
new = {k: v for k, v in b["entries"].items() if k not in a["entries"]}
a["entries"].update(new)
json.dump(a, open("$O/tuned_merged_r4.json", "w"), indent=0)
print("new shapes:", len(new)); [print("  ", k, v) for k, v in new.items()]
PYEOF
  grep -o '"tuned_live": [0-9]*' $O/tunemissing.json $O/tunemissing_sd15.json $O/tunemissing_flux.json
fi
if [[ $WHAT == *pfab* ]]; then
  for cap in 16 0 16 0; do
    DIFFUSERS_AMD_PREFETCH_CAP_MB=$cap timeout 600 python bench.py --steps 3 --warmup 1 --no-reference --no-cpu-baseline --no-roofline --no-other-configs > $O/bench_pf$cap.json 2> $O/bench_pf$cap.err; echo "prefetch cap $cap MB rc=$? $(cut -c1-140 $O/bench_pf$cap.json | grep -o '"value": [0-9.]*')"
  done
fi
if [[ $WHAT == *xcd* ]]; then
  rm -f $O/xcd_r4.jsonl
  for gx in auto 1 2 4 8; do
    if [[ $gx == auto ]]; then timeout 120 python tools/bench_xcd_r4.py $O/xcd_r4.jsonl > $O/xcd_r4.log 2>&1; else DA_XCD_GX=$gx timeout 120 python tools/bench_xcd_r4.py $O/xcd_r4.jsonl >> $O/xcd_r4.log 2>&1; fi
  done
  cat $O/xcd_r4.jsonl
  for gx in 1 4; do
    DA_XCD_GX=$gx timeout 600 python bench.py --steps 3 --warmup 1 --no-reference --no-cpu-baseline --no-roofline --no-other-configs > $O/bench_gx$gx.json 2> $O/bench_gx$gx.err; echo "DA_XCD_GX=$gx rc=$? $(cut -c1-140 $O/bench_gx$gx.json | grep -o '"value": [0-9.]*')"
  done
  timeout 600 python bench.py --steps 3 --warmup 1 --no-reference --no-cpu-baseline --no-roofline --no-other-configs > $O/bench_gxauto.json 2> $O/bench_gxauto.err; echo "auto rc=$? $(cut -c1-140 $O/bench_gxauto.json | grep -o '"value": [0-9.]*')"
fi
if [[ $WHAT == *pmcshapes* ]]; then
  cd /tmp && export TMPDIR=/tmp
  rm -rf $O/pmc_shapes; mkdir -p $O/pmc_shapes
  : > $O/r04_fetch_by_shape.md
  for gx in auto 1 8; do
    if [[ $gx == auto ]]; then unset DA_XCD_GX; else export DA_XCD_GX=$gx; fi
    DIFFUSERS_AMD_TUNE=0 timeout 200 rocprofv3 --kernel-trace --pmc FETCH_SIZE -f csv -d $O/pmc_shapes/gx$gx -o s -- python $R/tools/pmc_shapes_r4.py run $O/pmc_shapes/manifest_$gx.json > $O/pmc_shapes/gx$gx.log 2>&1; echo "pmc shapes gx=$gx rc=$?"
    python $R/tools/pmc_shapes_r4.py report $O/pmc_shapes/manifest_$gx.json $(find $O/pmc_shapes/gx$gx -name '*counter_collection.csv') >> $O/r04_fetch_by_shape.md 2>> $O/pmc_shapes/gx$gx.log
    echo >> $O/r04_fetch_by_shape.md
  done
  unset DA_XCD_GX
  find $O/pmc_shapes -name '*kernel_trace*' -delete
  cd $R
  cat $O/r04_fetch_by_shape.md
fi
if [[ $WHAT == *qkv* ]]; then
  timeout 600 python -m pytest tests/test_gemm_k2_gpu.py -m gpu -q -s --timeout 300 -k "fused_qkv or layernorm_fold" > $O/pytest_qkv.log 2>&1; echo "pytest qkv rc=$?"
  grep -E "passed|failed|FAILED|Error|assert" $O/pytest_qkv.log | tail -12
  rm -f $O/qkv_r4.jsonl
  timeout 300 python tools/bench_qkv_r4.py $O/qkv_r4.jsonl > $O/qkv_r4.log 2>&1; echo "qkv bench rc=$?"; tail -3 $O/qkv_r4.log | cut -c1-300
  cat $O/qkv_r4.jsonl
  # the shipped table's choice, then the whole field (both kernel families) measured again in situ
  for rt in 0 1 0 1; do
    DIFFUSERS_AMD_QKV_RETUNE=$rt DIFFUSERS_AMD_GEMM_FAMILY=all DIFFUSERS_AMD_TUNE_SAVE=$O/tuned_qkv_rt$rt.json timeout 600 python bench.py --steps 3 --warmup 1 --no-reference --no-cpu-baseline --no-roofline --no-other-configs > $O/bench_rt_$rt.json 2> $O/bench_rt_$rt.err; echo "qkv retune $rt rc=$? $(cut -c1-140 $O/bench_rt_$rt.json | grep -o '"value": [0-9.]*') $(grep -o '"tuned_live": [0-9]*' $O/bench_rt_$rt.json)"
  done
  python - <<PYEOF
import json
try:
    b = json.load(open("$O/tuned_qkv_rt1.json"))
    print({k: v for k, v in b["entries"].items() if k.startswith("qkv:")})
except Exception as e:
    print("no table:", e)
PYEOF
  for n1 in; do
    DIFFUSERS_AMD_LN_FOLD_NORM1=$n1 DIFFUSERS_AMD_TUNE_SAVE=$O/tuned_qkv_r4.json timeout 600 python bench.py --steps 3 --warmup 1 --no-reference --no-cpu-baseline --no-roofline --no-other-configs > $O/bench_n1_$n1.json 2> $O/bench_n1_$n1.err; echo "norm1 fold $n1 rc=$? $(cut -c1-140 $O/bench_n1_$n1.json | grep -o '"value": [0-9.]*') $(grep -o '"tuned_live": [0-9]*' $O/bench_n1_$n1.json)"
  done
  python - <<PYEOF
import json
try:
    b = json.load(open("$O/tuned_qkv_r4.json"))
    print({k: v for k, v in b["entries"].items() if k.startswith("qkv:")})
except Exception as e:
    print("no table:", e)
PYEOF
fi
if [[ $WHAT == *modeab* ]]; then
  for mode in 2 1 2 1; do
    DIFFUSERS_AMD_LN_FOLD=$mode timeout 600 python bench.py --steps 3 --warmup 1 --no-reference --no-cpu-baseline --no-roofline --no-other-configs > $O/bench_mode$mode.json 2> $O/bench_mode$mode.err; echo "fold mode $mode rc=$? $(cut -c1-140 $O/bench_mode$mode.json | grep -o '"value": [0-9.]*') $(grep -o '"tuned_live": [0-9]*' $O/bench_mode$mode.json)"
  done
fi
if [[ $WHAT == *pmcattn* ]]; then
  cd /tmp && export TMPDIR=/tmp
  rm -rf $O/pmc_attn; mkdir -p $O/pmc_attn
  timeout 300 rocprofv3 --kernel-trace --pmc SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_VALU_MFMA_BUSY_CYCLES SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE -f csv -d $O/pmc_attn/sq -o a -- python $R/tools/pmc_attn_r4.py run $O/pmc_attn/manifest.json > $O/pmc_attn/sq.log 2>&1; echo "pmc attn rc=$?"
  cd $R
  python tools/pmc_attn_r4.py report $O/pmc_attn/manifest.json $(find $O/pmc_attn/sq -name '*counter_collection.csv' | head -1) > $O/r04_pmc_attention.md 2>> $O/pmc_attn/sq.log
  find $O/pmc_attn -name '*kernel_trace*' -delete
  cat $O/r04_pmc_attention.md | cut -c1-330; tail -2 $O/pmc_attn/sq.log | cut -c1-200
fi
if [[ $WHAT == *tuneothers* ]]; then
  # shapes of the other BASELINE configs that the shipped table does not hold (bench.py reports them as config.tuned_live)
  rm -f $O/tuned_others_r4.json
  for cfg in sd15 flux ddpm; do
    DIFFUSERS_AMD_GEMM_FAMILY=all DIFFUSERS_AMD_TUNE_SAVE=$O/tuned_others_r4.json timeout 600 python bench.py --full --config $cfg --steps 1 --warmup 1 --no-cpu-baseline > $O/tuneothers_$cfg.json 2>> $O/tuneothers.err; echo "tuneothers $cfg rc=$? $(grep -o '"tuned_live": [0-9]*' $O/tuneothers_$cfg.json)"
    python - <<PYEOF
import json
a = json.load(open("$R/diffusers_amd/tuned/gfx950.json"))
try:
    b = json.load(open("$O/tuned_others_r4.json"))
except Exception as e:
    b = {"entries": {}}
print("  new after $cfg:", {k: v for k, v in b["entries"].items() if k not in a["entries"]})
PYEOF
  done
fi
if [[ $WHAT == *planbench* ]]; then
  rm -f $O/plan_r4.jsonl
  timeout 600 python tools/bench_plan_r4.py $O/plan_r4.jsonl > $O/plan_r4.log 2>&1; echo "plan bench rc=$?"; tail -3 $O/plan_r4.log | cut -c1-900
fi
if [[ $WHAT == *profothers* ]]; then
  cd /tmp && export TMPDIR=/tmp
  for cfg in sd15 ddpm; do
    rm -rf $O/prof_$cfg
    timeout 600 rocprofv3 --kernel-trace --stats -f csv -d $O/prof_$cfg -o $cfg -- python $R/bench.py --full --config $cfg --steps 1 --warmup 1 --no-cpu-baseline > $O/prof_$cfg.log 2>&1; echo "prof $cfg rc=$?"
    find $O/prof_$cfg -name '*kernel_trace*' -size +30M -delete
    python $R/tools/prof_summary.py $(find $O/prof_$cfg -name '*kernel_stats.csv' | head -1) "r04 $cfg bench (--steps 1 --warmup 1)" > $O/prof_summary_$cfg.md 2>> $O/prof_$cfg.log; head -34 $O/prof_summary_$cfg.md | cut -c1-190
  done
  cd $R
fi
if [[ $WHAT == *retunesmall* ]]; then
  # the small-M, deep-K shapes of the SD1.5 / DDPM U-Nets (fewer tiles than CUs): tuned again with the split-K variants (2..8)
  # and both kernel families competing; SDXL's entries are left alone
  python - <<PYEOF
import json, re
R, O = "$R", "$O"
d = json.load(open(f"{R}/diffusers_amd/tuned/gfx950.json"))
sdxl = set(json.load(open(f"{R}/tests/golden/sdxl_gemm_shape_keys.json"))["keys"])
BM = {"128x128": (128, 128), "64x128": (64, 128), "128x64": (128, 64), "64x64": (64, 64), "256x128": (256, 128), "128x256": (128, 256),
      "256x256": (256, 256), "128x128w8": (128, 128), "k2:128x128": (128, 128), "k2:128x80": (128, 80), "k2:128x160": (128, 160),
      "k2:80x128": (80, 128), "k2:128x64": (128, 64), "k1:128x320": (128, 320), "k1:256x128": (256, 128), "k1:128x256": (128, 256),
      "k1:256x160": (256, 160), "k1:256x256": (256, 256), "k1:256x320": (256, 320)}
drop = []
for k, v in d["entries"].items():
    if k in sdxl or k.startswith(("pair:", "qkv:")):
        continue
    m = re.match(r"conv(\d):M(\d+):N(\d+):C(\d+)\+(\d+)", k)
    if m:
        ks, M, N, C1, C2 = map(int, m.groups()); K = ks * ks * (C1 + C2)
    else:
        m = re.match(r"lin:M(\d+):N(\d+):K(\d+)", k)
        if not m:
            continue
        M, N, K = map(int, m.groups())
    bm, bn = BM[d["tiles"][v[0]]]
    tiles = -(-M // bm) * -(-N // bn)
    if tiles < 200 and K >= 1024 and M <= 8192:
        drop.append(k)
for k in drop:
    del d["entries"][k]
json.dump(d, open(f"{O}/table_pruned.json", "w"))
print("entries to tune again:", len(drop))
PYEOF
  cp $O/table_pruned.json $O/table_retuned.json
  for cfg in sd15 ddpm; do
    DIFFUSERS_AMD_SPLITK=1 DIFFUSERS_AMD_GEMM_FAMILY=all DIFFUSERS_AMD_TUNE_DB=$O/table_retuned.json DIFFUSERS_AMD_TUNE_SAVE=$O/table_retuned.json timeout 900 python bench.py --full --config $cfg --steps 1 --warmup 1 --no-cpu-baseline > $O/retune_$cfg.json 2> $O/retune_$cfg.err; echo "retune $cfg rc=$? $(grep -o '"value": [0-9.]*' $O/retune_$cfg.json | head -1) $(grep -o '"tuned_live": [0-9]*' $O/retune_$cfg.json)"
  done
  python - <<PYEOF
import json
a = json.load(open("$R/diffusers_amd/tuned/gfx950.json"))["entries"]
b = json.load(open("$O/table_retuned.json"))
T = b["tiles"]
n = 0
for k, v in sorted(b["entries"].items()):
    o = a.get(k)
    if o is None or o[:2] != v[:2] or (len(v) > 3) != (len(o) > 3):
        n += 1
        print(f"  {k:58s} {T[o[0]] if o else '-':11s} st{o[1] if o else '-'} {o[2] if o else 0:7.1f}us -> {T[v[0]]:11s} st{v[1]} split {v[3] if len(v) > 3 else 1} {v[2]:7.1f}us")
print("changed:", n)
PYEOF
  for rep in 1 2; do
    for tb in $R/diffusers_amd/tuned/gfx950.json $O/table_retuned.json; do
      for cfg in sd15 ddpm; do
        DIFFUSERS_AMD_TUNE_DB=$tb timeout 600 python bench.py --config $cfg --steps 2 --warmup 1 --no-cpu-baseline --no-roofline > $O/ab_$cfg.json 2> $O/ab_$cfg.err; echo "$(basename $tb) $cfg rc=$? $(grep -o '"value": [0-9.]*' $O/ab_$cfg.json | head -1) $(grep -o '"tuned_live": [0-9]*' $O/ab_$cfg.json) $(grep -o '"psnr[a-z_]*": [0-9.]*' $O/ab_$cfg.json | head -2 | tr '\n' ' ')"
      done
    done
  done
fi
if [[ $WHAT == *tembab* ]]; then
  for rep in 1 2; do
    for st in 0 1; do
      for cfg in sdxl sd15 ddpm; do
        EXTRA="--no-reference --no-other-configs"; [[ $cfg != sdxl ]] && EXTRA=""
        DIFFUSERS_AMD_TEMB_STACK=$st timeout 600 python bench.py --config $cfg --steps 3 --warmup 1 --no-cpu-baseline --no-roofline $EXTRA > $O/temb_$cfg.json 2> $O/temb_$cfg.err; echo "stacked time projections $st $cfg rc=$? $(grep -o '"value": [0-9.]*' $O/temb_$cfg.json | head -1)"
      done
    done
  done
fi
