set -e
O=${1:?usage: tools/gpu_round.sh OUTDIR}
mkdir -p $O
python -m pytest tests -m gpu -x -q > $O/r02_gpu_all.txt 2>&1 || { tail -40 $O/r02_gpu_all.txt; exit 1; }
tail -2 $O/r02_gpu_all.txt
python bench.py --full 2>/dev/null | grep '^{' > $O/r02_bench_n1.json; cat $O/r02_bench_n1.json | cut -c1-400
python bench.py --gpus 1 --workload c5 --steps 20 --warmup 3 --full 2>/dev/null | grep '^{' > $O/r02_bench_c5_full_one_gpu.json; cut -c1-300 $O/r02_bench_c5_full_one_gpu.json
python tools/report.py $O/r02_report_all_configs.md 2>/dev/null | tail -8
KB_TIMG=1 python tools/kbench.py c2 500 T 2>/dev/null | tail -2 > $O/r02_c2_transposed.txt
python tools/kbench.py c2 500 T 2>/dev/null | tail -2 >> $O/r02_c2_transposed.txt
cat $O/r02_c2_transposed.txt
