JFSX_LIB=parent.so rocprofv3 --pmc TCP_TOTAL_CACHE_ACCESSES_sum TCP_TCC_READ_REQ_sum TCP_TOTAL_ACCESSES_sum -- python3 bench.py --steps 1 --warmup 0 --no-cpu --verify 0 --blocks 1024
