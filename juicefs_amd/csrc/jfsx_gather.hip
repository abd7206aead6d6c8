// jfsx_gather.hip -- gather_pages_k on gfx950: the pages of a compacted slice
// assembled in device memory from pieces of other pages and zeros
// (jfsx_gather_batch; stage 3 of jfsx_compact_objects).  One launch per call,
// whatever the number of pages and pieces: the grid is capped near 8
// workgroups per CU and strides over the tiles of all pages.  jfsx_gather.h has
// the per-lane arithmetic and the reasons for its shape; there is no LDS, no
// scratch and no inline assembly here.  Sources and destinations are device
// allocations, so their accesses are global ones (GlobalMem), not flat.
// Stores are plain: the next kernel of the chain (a page CRC, a compressor or
// the Seal) reads the page back.
#include "jfsx_internal.h"

#define JFSX_HD __device__ __forceinline__
#include "jfsx_gather.h"

namespace jfsx {

namespace {

#define JFSX_GLOBAL __attribute__((address_space(1)))
typedef uint32_t gather_v4 __attribute__((ext_vector_type(4)));
struct GlobalMem {
    __device__ __forceinline__ jfsx_gather::U4 ld16(const uint8_t *q) const {
        const gather_v4 v = *(const JFSX_GLOBAL gather_v4 *)q;
        return jfsx_gather::U4{v.x, v.y, v.z, v.w};
    }
    __device__ __forceinline__ void st16(uint8_t *q, jfsx_gather::U4 v) const {
        *(JFSX_GLOBAL gather_v4 *)q = gather_v4{v.x, v.y, v.z, v.w};
    }
    __device__ __forceinline__ uint8_t ld8(const uint8_t *q) const { return *(const JFSX_GLOBAL uint8_t *)q; }
    __device__ __forceinline__ void st8(uint8_t *q, uint8_t v) const { *(JFSX_GLOBAL uint8_t *)q = v; }
};

__global__ __launch_bounds__(jfsx_gather::kThreads) void gather_pages_k(
    uint32_t n_pages, uint64_t n_tiles, const jfsx_gather::GPage *__restrict__ pages,
    const jfsx_gather::GPiece *__restrict__ pieces) {
    GlobalMem m;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)
        jfsx_gather::gather_lane(pages, n_pages, pieces, tile, threadIdx.x, m);
}

}  // namespace

void launch_gather(hipStream_t s, int ncu, uint32_t n_pages, uint64_t n_tiles, const void *pages, const void *pieces) {
    if (!n_pages || !n_tiles) return;
    const uint64_t cap = (uint64_t)(ncu > 0 ? ncu : 256) * 8;
    const uint32_t grid = (uint32_t)(n_tiles < cap ? n_tiles : cap);
    hipLaunchKernelGGL(gather_pages_k, dim3(grid), dim3(jfsx_gather::kThreads), 0, s, n_pages, n_tiles,
                       static_cast<const jfsx_gather::GPage *>(pages),
                       static_cast<const jfsx_gather::GPiece *>(pieces));
}

}  // namespace jfsx
