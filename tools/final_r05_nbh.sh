O=${1:?usage: tools/final_r05_nbh.sh OUTPUT_DIR}
mkdir -p $O
python -m pytest tests -q -m gpu -x 2>&1 | grep -E "passed|failed|error" > $O/r05_pytest_gpu.txt
GPP_LIB=$PWD/gridpp_amd/lib/var_poison.so GRIDPP_TEST_POISON=1 python -m pytest tests -q -m gpu -x 2>&1 | grep -E "passed|failed|error" > $O/r05_pytest_gpu_poisoned.txt
GPP_LIB=$PWD/gridpp_amd/lib/var_poison.so python tools/nbh_hostile_soak.py 0 160 20 poison dump=/tmp/d > $O/r05_nbh_hostile_soak.txt 2>&1
python tools/qf_soak.py 2>&1 | grep -v amdgpu.ids > $O/r05_qf_soak.txt
python tools/march_soak.py 150 2>&1 | grep -v amdgpu.ids > $O/r05_march_soak.txt
python tools/neighbourhood_soak.py 2>&1 | grep -v amdgpu.ids > $O/r05_neighbourhood_soak.txt
PROFILE_ONLY=nbh bash tools/profile_r05.sh > /dev/null 2>&1
for f in $O/*.txt; do echo "== $f"; tail -n 2 $f; done
python tools/slice_overhead_other.py 2>&1 | grep -v amdgpu.ids > $O/r05_slice_overhead_other.txt
python bench.py --full > $O/r05_bench_n1_final.json 2> $O/bench.err
cut -c1-400 $O/r05_bench_n1_final.json
