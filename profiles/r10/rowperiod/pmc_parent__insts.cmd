JFSX_LIB=parent.so rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_LDS_IDX_ACTIVE -- python3 bench.py --steps 1 --warmup 0 --no-cpu --verify 0 --blocks 1024
