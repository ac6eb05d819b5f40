#!/bin/bash
# k_verify time per mixed addition across comb windows (cache-resident vs
# 258 GiB tables): one short bench per window pair.
# Output under $OUT_DIR (default bench_out/) in the repository.
cd "$(dirname "$0")/.." || exit 1
O=${OUT_DIR:-bench_out}
mkdir -p $O
for w in ${MBFT_PROBE_WINDOWS:-16 22 26 29}; do
  timeout -k 10 300 python bench.py --full --steps 20 --warmup 5 --g-window $w --q-window $w --no-cpu-baseline \
    --c3-requests 0 --no-adversarial > $O/bench_w$w.json 2> $O/bench_w$w.err || exit 1
done
