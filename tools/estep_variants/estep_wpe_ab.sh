#!/bin/bash
# A/B of SPM_HIP_ESTEP_WPE on the c4 E-step bench leg (bench.py --full).
# Output goes to $O (default: a fresh temporary directory).
R=${GRAFT_REPO_ROOT:-$(pwd)}
O=${O:-$(mktemp -d)}
mkdir -p $O
cd /tmp
for w in 2 3 4; do
  SPM_HIP_ESTEP_WPE=$w timeout -k 10 200 python3 $R/bench.py --full --steps 1 --warmup 1 --raw-steps 0 --train-lines 0 --no-cpu-baseline > $O/b$w.json 2> $O/e$w.txt || { tail -5 $O/e$w.txt; exit 1; }
  python3 -c "import json;d=json.load(open('$O/b$w.json'));print('wpe $w', d['estep']['value'])"
done
