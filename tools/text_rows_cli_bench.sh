#!/bin/bash
# Wall time of spm_encode over botchan repeated to ~1 M lines, id and piece
# format: device text rows (SPM_HIP_TEXT_ROWS unset) against the host path
# (=0) and, when PARENT_BIN names the parent commit's spm_encode, against
# that; alternated, three runs each.  usage: tools/text_rows_cli_bench.sh [outdir]
set -o pipefail
root=$(cd "$(dirname "$0")/.." && pwd)
out=${1:-/tmp}
bin=$root/sentencepiece-comments_amd/lib/spm_encode
model=$root/tests/golden/test_model.model
big=$out/botchan_1m.txt
: > "$big"
for i in $(seq 233); do cat "$root/tests/golden/botchan.txt" >> "$big"; done
echo "input: $(wc -l < "$big") lines, $(wc -c < "$big") bytes"
run() {  # label, binary, env assignment
  local t0=${EPOCHREALTIME/./}
  env $3 timeout -k 10 120 "$2" --model="$model" --output_format="$fmt" --output="$out/rows_$1.txt" "$big" || exit 1
  local t1=${EPOCHREALTIME/./}
  echo "$fmt $1 $(( (t1 - t0) / 1000 )) ms"
}
for fmt in id piece; do
  for rep in 1 2 3; do
    run device "$bin" SPM_HIP_TEXT_ROWS_TIMES=1
    run host "$bin" SPM_HIP_TEXT_ROWS=0
    if [ -n "$PARENT_BIN" ]; then run parent "$PARENT_BIN" SPM_HIP_TEXT_ROWS_UNUSED=1; fi
  done
  cmp "$out/rows_device.txt" "$out/rows_host.txt" && echo "$fmt: device and host outputs identical"
done
rm -f "$big" "$out"/rows_*.txt
