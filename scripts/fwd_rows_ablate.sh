#!/bin/bash
# Ablations of the whole-row attention forward kernel (diagnostic build, JMT_ATTN_FWD_ROWS_DBG
# bits: 2 no score reads / MFMAs, 4 no softmax, 8 no K / V DMA after tile 0, 16 no P V reads /
# MFMAs, 32 no O / lse stores; results wrong, timing only) at the c3 and c4 forward launches
# (scripts/bench_attn.py fwd-ab: the 64-row kernel of the same process is the fixed reference).
# Usage: scripts/fwd_rows_ablate.sh OUT [diag library]
OUT=${1:-profiles/r07/fwd_rows_ablate.txt}
LIB=${2:-joint-multimodal-transformer-6th-abaw_amd/jmt/libjmt_hip_diag.so}
mkdir -p "$(dirname "$OUT")"
for d in ${DBGS:-0 2 4 8 16 32 18 22 54 62}; do
  echo "JMT_ATTN_FWD_ROWS_DBG=$d" >> "$OUT"
  JMT_LIB=$LIB JMT_ATTN_FWD_ROWS_DBG=$d timeout -k 10 90 python -u scripts/bench_attn.py fwd-ab 3 \
    2>/dev/null | grep '^{' >> "$OUT" || exit 1
done
