#!/bin/bash
# round-5 check: new probes + co-residency test first, the GPU tier, smoke, tanh probe, bench
set -o pipefail
cd "$GRAFT_REPO_ROOT"
OUT=gpurun_out/${OUTD:-r5a}; mkdir -p $OUT
export TMPDIR=/tmp
step() { local n=$1; shift; echo "== $n"; timeout -k 10 ${T:-300} "$@" > $OUT/$n.log 2>&1; local rc=$?; tail -${TL:-3} $OUT/$n.log; return $rc; }
step new python -u -m pytest tests/test_gpu_probes.py tests/test_gpu_production.py -q -x --timeout 200 --timeout-method thread -k "probe or tanh or held" &&
TL=1 step tanh python -u tools/tanh_probe.py &&
step gemmt python -u -m pytest tests/test_gpu_gemm.py -q -x --timeout 120 --timeout-method thread &&
TL=8 step gemm python -u tools/gemm_micro.py &&
T=900 step tier python -u -m pytest tests -m gpu -q -x --timeout 300 --timeout-method thread &&
step smoke python -u -c "import __graft_entry__ as g; g.smoke()" &&
T=600 TL=1 step bench python -u bench.py --full &&
step trace rocprofv3 --kernel-trace -d $OUT/tr -o run --output-format csv -- python3 bench.py --full --steps 2 --warmup 1 --decode-batches 0 --config5-steps 0 &&
python scripts/kwin.py $OUT/tr/run_kernel_trace.csv 1 40 > $OUT/kwin_b256.txt &&
python scripts/loop_tl.py $OUT/tr/run_kernel_trace.csv attn_bwd_rowp 60 30 > $OUT/tl_bwd.txt &&
python scripts/loop_tl.py $OUT/tr/run_kernel_trace.csv attn_fwd_rowp 60 30 > $OUT/tl_fwd.txt &&
rm -rf $OUT/tr && echo done
for v in 1 0 1 0; do
  TSAMD_VL_STORE=$v T=120 step vl$v rocprofv3 --kernel-trace --stats -d $OUT/v$v -o run --output-format csv -- python3 tools/vocab_micro.py || exit 1
  python scripts/kstats.py $OUT/v$v/run_kernel_stats.csv 1 3 | sed -n 2,3p
done
