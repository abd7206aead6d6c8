// Table-lookup throughput probe (measurement tool, not product code).
// T-table AES-256 is bound by LDS lookups (2 LDS cycles per wave64
// ds_read_b32): this measures how many random 32-bit lookups per clock per CU
// the other paths deliver -- global loads that hit the vector L1 (a 1 or 4 KiB
// table), and mixes of LDS and L1 lookups in one wave -- so the GCM kernel
// can decide whether moving part of its lookups to the L1 pays.
// Each lane runs CH independent chains x <- rotl8(x) ^ T[byte(x)] (the shape
// of an AES column), 16 waves per CU, one workgroup per CU.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#define CH 8
#define WAVES 16
typedef __attribute__((address_space(1))) const uint32_t gu32;
typedef __attribute__((address_space(3))) const uint32_t lu32;

__device__ __forceinline__ uint32_t rotl8(uint32_t x) { return __builtin_amdgcn_alignbit(x, x, 24); }

// MODE 0: LDS only (replicated, conflict-free); 1: L1 only, 1 KiB table;
// 2: L1 only, 4 KiB table (byte k of x picks sub-table k);
// 3: 2 LDS : 1 L1; 4: 1 LDS : 1 L1; 5: 3 LDS : 1 L1; 6: L1 only, 16 KiB
// (modes 7 and 8, the side-gather pair, are probe_side below)
template <int MODE>
__global__ __launch_bounds__(WAVES * 64) void probe(const uint32_t *__restrict__ gtab, uint32_t *out, uint32_t seed,
                                                    int iters) {
    __shared__ uint32_t lds[256 * 64];  // entry idx at byte idx*256 + 4*replica (as the GCM kernel's T0|T2)
    for (uint32_t i = threadIdx.x; i < 256 * 64; i += blockDim.x) lds[i] = gtab[i >> 6];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t loff = (lane & 31) << 2;
    gu32 *g = (gu32 *)gtab;
    lu32 *l = (lu32 *)lds;
    uint32_t x[CH];
#pragma unroll
    for (int i = 0; i < CH; i++) x[i] = seed * (threadIdx.x + 1 + 64 * blockIdx.x) + i * 0x9e3779b9u;
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int i = 0; i < CH; i++) {
            // byte 0 of x as the index; the LDS address (idx << 7) | replica
            const uint32_t la = __builtin_amdgcn_perm(x[i], loff, 0x0c0c0400u);  // (b0 << 8) | loff
            const uint32_t ga = (x[i] & 0xffu) << 2;
            uint32_t v;
            if constexpr (MODE == 0) v = *(const lu32 *)((const __attribute__((address_space(3))) char *)l + la);
            else if constexpr (MODE == 1) v = *(gu32 *)((__attribute__((address_space(1))) const char *)g + ga);
            else if constexpr (MODE == 2) v = *(gu32 *)((__attribute__((address_space(1))) const char *)g + ga + ((i & 3) << 10));
            else if constexpr (MODE == 6) v = *(gu32 *)((__attribute__((address_space(1))) const char *)g + ga + ((i & 15) << 10));
            else {
                constexpr int per = MODE == 3 ? 3 : (MODE == 4 ? 2 : 4);  // one L1 lookup per `per`
                if (i % per == per - 1) v = *(gu32 *)((__attribute__((address_space(1))) const char *)g + ga);
                else v = *(const lu32 *)((const __attribute__((address_space(3))) char *)l + la);
            }
            x[i] = rotl8(x[i]) ^ v;
        }
    }
    uint32_t r = 0;
#pragma unroll
    for (int i = 0; i < CH; i++) r ^= x[i];
    out[blockIdx.x * blockDim.x + threadIdx.x] = r;
}

// Side gathers (modes 7 and 8): the GCM row loop's mix when the fused CRC's
// data-only slice lookups leave the LDS.  One body is 197 dependent LDS
// lookups (24 steps of the CH chains and 5 more lookups: the AES, GHASH and
// remaining CRC reads of one 1 KiB row) and, with SIDE, 12 L1 gathers beside
// them: slice tables 4..15 of a 16 KiB image indexed by the bytes of three
// data words that depend on no lookup.  A gather is issued every second step
// and XOR-folded one step (8 LDS lookups per lane) later, so it sits on no
// chain and one is in flight.  The rate reported is LDS lookups per clock; the pair runs back
// to back so the two figures share one clock state.
template <bool SIDE>
__global__ __launch_bounds__(WAVES * 64) void probe_side(const uint32_t *__restrict__ gtab, uint32_t *out,
                                                         uint32_t seed, int iters) {
    __shared__ uint32_t lds[256 * 64];
    for (uint32_t i = threadIdx.x; i < 256 * 64; i += blockDim.x) lds[i] = gtab[i >> 6];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t loff = (lane & 31) << 2;
    const __attribute__((address_space(1))) char *g = (const __attribute__((address_space(1))) char *)gtab;
    const __attribute__((address_space(3))) char *l = (const __attribute__((address_space(3))) char *)lds;
    uint32_t x[CH];
#pragma unroll
    for (int i = 0; i < CH; i++) x[i] = seed * (threadIdx.x + 1 + 64 * blockIdx.x) + i * 0x9e3779b9u;
    uint32_t d[3] = {x[0] * 0x85ebca6bu, x[1] * 0xc2b2ae35u, x[2] * 0x27d4eb2fu};
    uint32_t side = 0;
#define LDS_STEP(i) x[i] = rotl8(x[i]) ^ *(const lu32 *)(l + __builtin_amdgcn_perm(x[i], loff, 0x0c0c0400u))
    for (int it = 0; it < iters; it++) {
        uint32_t v[12];
#pragma unroll
        for (int st = 0; st < 24; st++) {
            if (SIDE && st % 2 == 0) {
                const int k = st / 2;  // table 4 + k, byte k & 3 of data word k / 4
                v[k] = *(gu32 *)(g + (((d[k >> 2] >> (8 * (k & 3))) & 0xffu) << 2) + 1024 * (4 + k));
            }
#pragma unroll
            for (int i = 0; i < CH; i++) LDS_STEP(i);
            if (SIDE && st % 2 == 1) side ^= v[st / 2];
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int i = 0; i < 5; i++) LDS_STEP(i);
        // the next row's data: a function of the row number alone
#pragma unroll
        for (int k = 0; k < 3; k++) d[k] = d[k] * 0x9e3779b1u + (uint32_t)it;
    }
#undef LDS_STEP
    uint32_t r = side ^ d[0] ^ d[1] ^ d[2];
#pragma unroll
    for (int i = 0; i < CH; i++) r ^= x[i];
    out[blockIdx.x * blockDim.x + threadIdx.x] = r;
}

typedef void (*kfn)(const uint32_t *, uint32_t *, uint32_t, int);

int main() {
    kfn fns[] = {probe<0>, probe<1>, probe<2>, probe<3>, probe<4>, probe<5>, probe<6>};
    const char *names[] = {"LDS ds_read_b32 (32 replicas)", "L1 global_load_dword, 1 KiB table",
                           "L1 global_load_dword, 4 KiB table", "2 LDS : 1 L1", "1 LDS : 1 L1", "3 LDS : 1 L1",
                           "L1 global_load_dword, 16 KiB table"};
    hipDeviceProp_t prop;
    hipGetDeviceProperties(&prop, 0);
    const int cus = prop.multiProcessorCount;
    uint32_t *tab, *out;
    hipMalloc(&tab, 16384 * 4);
    hipMalloc(&out, (size_t)cus * 4 * WAVES * 64 * 4);
    uint32_t h[16384];
    for (int i = 0; i < 16384; i++) h[i] = 0x9e3779b9u * (i + 1) ^ (i << 13);
    hipMemcpy(tab, h, sizeof h, hipMemcpyHostToDevice);
    const int iters = 4096;
    hipEvent_t a, b;
    hipEventCreate(&a);
    hipEventCreate(&b);
    printf("CUs %d, clock %d kHz; lookups per clock per CU at 2.4 GHz\n", cus, prop.clockRate);
    for (int m = 0; m < 7; m++) {
        for (int grid_mul = 1; grid_mul <= 2; grid_mul++) {
            const int grid = cus * grid_mul;
            hipLaunchKernelGGL(fns[m], dim3(grid), dim3(WAVES * 64), 0, 0, tab, out, 7u, 64);
            hipEventRecord(a);
            hipLaunchKernelGGL(fns[m], dim3(grid), dim3(WAVES * 64), 0, 0, tab, out, 7u, iters);
            hipEventRecord(b);
            hipEventSynchronize(b);
            float ms;
            hipEventElapsedTime(&ms, a, b);
            const double lookups = (double)grid * WAVES * 64 * CH * iters;
            printf("%-36s grid %4d: %8.3f ms  %.2f lookups/clk/CU (%.1f G lookups/s)\n", names[m], grid, ms,
                   lookups / (ms * 1e-3) / cus / 2.4e9, lookups / (ms * 1e-3) / 1e9);
        }
    }
    // the side-gather pair: one workgroup per CU, one timed run each
    const int side_iters = 256;
    double rate[2];
    for (int m = 0; m < 2; m++) {
        kfn f = m ? probe_side<true> : probe_side<false>;
        hipLaunchKernelGGL(f, dim3(cus), dim3(WAVES * 64), 0, 0, tab, out, 7u, 8);
        hipEventRecord(a);
        hipLaunchKernelGGL(f, dim3(cus), dim3(WAVES * 64), 0, 0, tab, out, 7u, side_iters);
        hipEventRecord(b);
        hipEventSynchronize(b);
        float ms;
        hipEventElapsedTime(&ms, a, b);
        const double lookups = (double)cus * WAVES * 64 * 197 * side_iters;
        rate[m] = lookups / (ms * 1e-3) / cus / 2.4e9;
        printf("%-36s grid %4d: %8.3f ms  %.2f LDS lookups/clk/CU%s\n",
               m ? "197 LDS + 12 side L1 gathers" : "197 LDS, no side gathers", cus, ms, rate[m],
               m ? " (+ 12/197 of that in L1 gathers)" : "");
    }
    printf("side gathers change the LDS lookup rate by %+.2f %% (they would free 13 %% of the row's LDS cycles)\n",
           100.0 * (rate[1] / rate[0] - 1.0));
    return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}
