#!/bin/bash
# Structure of the attention sources in two trees (profiles/attn_shared_parts.txt, step 1):  scratch/attn_shared_parts_structure.sh PARENT_TREE NEW_TREE
# Per file: lines, comment lines (text starts with //), and where the transposing-read builtin, the zero-fill offset and the three
# swizzle bit expressions are spelled out.
for tree in "$1" "$2"; do
  echo "== $tree"
  cd "$tree/autoregressive_diffusion_amd/csrc" || exit 1
  tl=0; tc=0
  for f in attention.hip attention_parts.h attention_ws.h attention_bwd_ws.h attention_bwd_dq_ws.h attention_frame.h; do
    [ -f $f ] || continue
    l=$(wc -l < $f); c=$(grep -c '^\s*//' $f); tl=$((tl + l)); tc=$((tc + c))
    printf "  %-26s %5d lines, %4d comment lines\n" $f $l $c
  done
  printf "  %-26s %5d lines, %4d comment lines\n" total $tl $tc
  for pat in 'ds_read_tr16_b64' '0x80000000' '>> 1) & 7' '4 \* ((\w* >> 1) & 1)' '>> 1) & 1) << 2' 'frame_burst512' 'exp2f(s\[kt\]\[rr\] - SOFTMAX_OFF)' 'exp2f(s\[rr\] - lse\(\[j\]\)\?) \* (dp\[rr\] - delta' 'const int qb4 = t \* 64 + qt \* 32'; do
    printf "  %-58s %s\n" "'$pat'" "$(grep -c -- "$pat" attention.hip attention_parts.h attention_ws.h attention_bwd_ws.h attention_bwd_dq_ws.h attention_frame.h 2>/dev/null | grep -v ':0$' | tr '\n' ' ')"
  done
  cd - > /dev/null
done
