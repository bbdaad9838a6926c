#!/bin/bash
# decode attention split-count sweep at B=1 (tuning aid)
for NS in 2 4 8 16; do
  EMMAX_ATTN_NSPLIT=$NS timeout 300 python bench.py --full --no-cpu-baseline --steps 1 --warmup 1 2>/dev/null | tail -1 | python -c "import json, sys; d=json.loads(sys.stdin.read()); print('nsplit', $NS, 'ms/token', d['decode_ms_per_token'], 'attn us', d['stage_us']['paged_attn'], 'oproj us', d['stage_us']['oproj_gemv'])"
done
