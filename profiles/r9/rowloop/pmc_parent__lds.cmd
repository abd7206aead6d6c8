JFSX_LIB=parent.so rocprofv3 --pmc SQ_LDS_IDX_ACTIVE SQ_LDS_BANK_CONFLICT SQ_INSTS_VALU SQ_INSTS_VMEM -- python3 bench.py --steps 1 --warmup 0 --no-cpu --verify 0 --blocks 1024
