set -e
# usage (GPU box, repository root): bash tools/collect_round.sh <out dir>; then python tools/summarize_profile.py <out dir> profiles/<name>
OUT=${1:?usage: bash tools/collect_round.sh <out dir>}
mkdir -p $OUT
python bench.py --full > $OUT/bench_cfg2_full.json 2> $OUT/bench_cfg2_full.err
echo "bench done"
export PROFILE_DIR=$OUT                                      # tools/profile.sh writes its passes next to everything else
bash tools/profile.sh "$(basename $OUT)" cfg2 > $OUT/profile_cfg2.log 2>&1; echo "cfg2 done"
bash tools/profile.sh "$(basename $OUT)" cfg3 > $OUT/profile_cfg3.log 2>&1; echo "cfg3 done"
bash tools/profile.sh "$(basename $OUT)" cfg4 > $OUT/profile_cfg4.log 2>&1; echo "cfg4 done"
bash tools/slice_prof.sh $OUT/slice cfg2 > $OUT/slice_prof.txt 2>&1; echo "slice prof done"
bash tools/slice_pmc.sh $OUT/slice_pmc cfg2 > $OUT/slice_pmc.txt 2>&1; echo "slice pmc done"
python tools/stage_alone.py cfg2 > $OUT/alone_cfg2.log 2>&1; python tools/stage_alone.py cfg4 > $OUT/alone_cfg4.log 2>&1; echo "alone done"
export MGACBAM_LIB=$PWD/build/variants/libmgacbam_trace.so
python tools/trace_gate.py fwd > $OUT/trace_k_gate.txt 2>&1
python tools/trace_gate.py bwd > $OUT/trace_k_bwd_apply.txt 2>&1
python tools/trace_gate.py pool > $OUT/trace_k_pool.txt 2>&1
python tools/trace_r12.py cfg2 > $OUT/trace_k_bwd_r12.txt 2>&1
python tools/trace_r12.py cfg3 > $OUT/trace_k_bwd_r12_cfg3.txt 2>&1
python tools/trace_head.py fwd > $OUT/trace_head_fwd.txt 2>&1
python tools/trace_head.py gx > $OUT/trace_head_gx.txt 2>&1
echo "traces done"
