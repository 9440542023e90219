#!/bin/bash
# Structure of the attention prologue in two trees (profiles/qkv_shared_parts.txt, step 1):  scratch/qkv_parts_structure.sh PARENT_TREE NEW_TREE
# Per file: lines and code lines (neither blank nor a // comment), and on how many lines the head norm's epsilon, the folded softmax
# scale, the 8-lane reduce, the adjoint's k2 and the KV-ring address are spelled out.
for tree in "$1" "$2"; do
  echo "== $tree"
  cd "$tree/autoregressive_diffusion_amd/csrc" || exit 1
  tl=0; tc=0
  for f in attention.hip attention_qkv.h; do
    [ -f $f ] || continue
    l=$(wc -l < $f); c=$(grep -cv '^\s*\(//.*\)\?$' $f); tl=$((tl + l)); tc=$((tc + c))
    printf "  %-22s %5d lines, %5d code lines\n" $f $l $c
  done
  printf "  %-22s %5d lines, %5d code lines\n" total $tl $tc
  for pat in '1e-4f' 'SCALE_LOG2 : 1.f' '__shfl_xor(\w*, 1).*__shfl_xor(\w*, 2).*__shfl_xor(\w*, 4)' 'sden \* sden \* n' 'kv_bstride + (kv_off'; do
    printf "  %-62s %s\n" "'$pat'" "$(grep -c -- "$pat" attention.hip attention_qkv.h 2>/dev/null | grep -v ':0$' | tr '\n' ' ')"
  done
  cd - > /dev/null
done
