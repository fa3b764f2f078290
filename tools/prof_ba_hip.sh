set -o pipefail
TAG=$1
OUT=${SFMX_PROF_DIR:-prof_out}/$TAG
mkdir -p $OUT
timeout -k 10 300 rocprofv3 --kernel-trace --hip-runtime-trace --output-format csv -d $OUT/prof_hip -o run -- python bench.py --full --only-ba --no-cpu-baseline > $OUT/prof_hip.log 2>&1
echo rc=$?
