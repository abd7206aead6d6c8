JFSX_LIB=libjfsx.so rocprofv3 --pmc SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_LDS SQ_BUSY_CYCLES -- python3 bench.py --steps 1 --warmup 0 --no-cpu --verify 0 --blocks 1024
