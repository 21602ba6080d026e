#!/bin/bash
# Round-end evidence on the GPU box (from the repo root): the full GPU suite, every rocprofv3 pass of tools/collect_profiles.sh,
# then the full bench line (bench.py --full).   tools/run_round_end.sh <tag>      Output: $RESULTS_DIR (default results/) + collect_profiles.sh's
tag=${1:-r04}
cd ${GRAFT_REPO_ROOT:-$(pwd)}
res=${RESULTS_DIR:-results}; mkdir -p $res
timeout 2400 python -m pytest tests -x -q -m gpu > $res/${tag}_gpu_tests.log 2>&1; tail -2 $res/${tag}_gpu_tests.log
bash tools/collect_profiles.sh $tag > $res/collect_${tag}.log 2>&1
cd ${GRAFT_REPO_ROOT:-$(pwd)}
python bench.py --full > $res/${tag}_bench.json 2> $res/${tag}_bench.err; tail -c 400 $res/${tag}_bench.json
