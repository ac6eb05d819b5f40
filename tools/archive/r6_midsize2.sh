#!/bin/bash
# Round 6: message-layer GPU tests, then the mid-size pass timeline again
# (one packed result copy, single-stream uploads, prefetched arena blocks).
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
O=gpurun_out/${R6TAG:-r6s}
mkdir -p $O
timeout -k 10 900 python -u -m pytest -x -q --timeout 240 --timeout-method thread tests/test_gpu_msgdev.py tests/test_gpu_multi_msg.py tests/test_gpu_check_coalesce.py tests/test_gpu_small_check.py tests/test_gpu_authen.py tests/test_gpu_sha.py tests/test_gpu_replies_go.py > $O/pytest.log 2>&1 || { tail -40 $O/pytest.log; exit 1; }
tail -2 $O/pytest.log
for w in 1024 4096; do
  LOWLOAD_SIZES=$w LOWLOAD_NREQ=1024 LOWLOAD_SMALL_MAX=0 timeout -k 10 300 rocprofv3 --kernel-trace --memory-copy-trace -d $O/t$w -o t --output-format csv -- python3 tools/lowload_probe.py > $O/lowload_$w.json 2> $O/lowload_$w.err || { tail -20 $O/lowload_$w.err; exit 1; }
  python3 tools/pass_timeline.py $O/t$w > $O/timeline_$w.json
  rm -f $(find $O/t$w -name "*kernel_trace.csv") $(find $O/t$w -name "*memory_copy_trace.csv")
done
LOWLOAD_SIZES=1024,2048,4096 LOWLOAD_NREQ=1024 LOWLOAD_SMALL_MAX=0 timeout -k 10 300 python3 tools/lowload_probe.py > $O/lowload_mid.json 2> $O/lowload_mid.err || { tail -20 $O/lowload_mid.err; exit 1; }
python3 -c "
import json; d=json.load(open('$O/lowload_mid.json'))
print({k:(round(v['p50_us'],1), round(v.get('cpu_us_per_window',0),1)) for k,v in d['go_default']['small_route'].items()})"
echo "[r6_midsize2] done"
