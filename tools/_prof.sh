# Round profile refresh on one MI355X: GPU tests, smoke, PMC traffic passes, kernel-trace stats, bench line.
# usage: bash tools/_prof.sh <tag> [out_dir]      (outputs under <out_dir>/<tag>_*, default prof_out)
set -e
T=${1:-v7}
O=${2:-prof_out}
mkdir -p $O
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $O/${T}_tests.log 2>&1
timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke()" > $O/${T}_smoke.log 2>&1
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
B="python3 bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-kernel-timing"
timeout -s KILL 180 rocprofv3 --pmc FETCH_SIZE -d $O/${T}f -o run --output-format csv -- $B > $O/${T}_pmcf.log 2>&1
timeout -s KILL 180 rocprofv3 --pmc WRITE_SIZE -d $O/${T}w -o run --output-format csv -- $B > $O/${T}_pmcw.log 2>&1
python tools/pmc_traffic.py $O/${T}f $O/${T}w $O/r01_${T}_pmc_traffic "round 1 ${T}: bench.py --steps 2 --warmup 1"
cp $O/r01_${T}_pmc_traffic.json profiles/
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/${T}s -o run --output-format csv -- python3 bench.py --steps 5 --warmup 1 --no-cpu-baseline --no-kernel-timing > $O/${T}_stats.log 2>&1
timeout -k 10 600 python bench.py --full > $O/${T}_bench.json 2> $O/${T}_bench.err
