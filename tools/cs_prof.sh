# bash tools/cs_prof.sh: stage cycles of corner_select_kernel (sequence 0's workgroup) during the bench's front-end steps
cd "$(dirname "$0")/.."
VIO_AMD_CS_PROF=1 python bench.py --quick --no-cpu-baseline --only frontend --steps 4 --warmup 2 2>&1 | grep "corner_select cycles" | tail -3
