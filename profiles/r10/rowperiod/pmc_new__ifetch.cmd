JFSX_LIB=libjfsx.so rocprofv3 --pmc SQ_IFETCH SQ_WAIT_IFETCH SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS -- python3 bench.py --steps 1 --warmup 0 --no-cpu --verify 0 --blocks 1024
