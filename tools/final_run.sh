set -e
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
O=${1:?usage: bash tools/final_run.sh OUTDIR}
mkdir -p $O
python -m pytest tests -m gpu -x -q > $O/pytest_gpu.txt 2>&1; tail -2 $O/pytest_gpu.txt
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $O/smoke.txt 2>&1; tail -1 $O/smoke.txt
python bench.py --full --steps 30 --warmup 5 > $O/bench.json 2> $O/bench.err
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -- python3 bench.py --full --steps 20 --warmup 3 --no-cpu-baseline --no-extras > $O/bench_profiled.json 2> $O/bench_profiled.err
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_train -- python3 tools/train_step_bench.py --iters 20 > $O/train_profiled.txt 2>&1
python3 tools/train_step_bench.py --graph --iters 20 > $O/train_bench.txt 2>&1
python bench.py --full --grid 128 --batch 32 --points 120000 --steps 10 --warmup 2 --no-cpu-baseline > $O/c3_bench.json 2> $O/c3.err
python tools/dropin_forward_bench.py > $O/dropin.txt 2>&1 || true
python tools/c4_bench.py > $O/c4.txt 2>&1 || true
echo done
