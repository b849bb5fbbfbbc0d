# OUT: the folder reproduce_profiles.sh fills for RTAG r05; the sf16 bench line goes there too
O=${OUT:?set OUT to the output folder of reproduce_profiles.sh for RTAG r05}
STEPS="1 3 4 5 7 8 9" ./tools/reproduce_profiles.sh > gpurun_out/regen_log.txt 2>&1
python bench.py --full --workload cfg3_qcnn_sf16_b256_bf16 --no-extras --no-cpu-baseline --no-standalone > "$O/r05_bench_sf16_builder_run.json" 2>/dev/null
tail -5 gpurun_out/regen_log.txt
