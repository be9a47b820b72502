// Microbenchmark: what does a 32-byte read at the head of an otherwise untouched 128-byte line cost?  The member-lines copy gave
// every UE a tail LINE of which the owner lane reads the first 32 bytes; the packed copy puts those 32 bytes of all UEs of a tile
// into one tail BLOCK ("Member lines").  Three patterns over a 1 GiB buffer (nothing is served by the Infinity Cache),
// every address read at most once per launch, non-temporal 16-byte buffer loads as the step kernel issues them:
//   (i)   calibration: whole lines, a cluster of eight lanes x 16 B per line, four consecutive lines per random 512-byte row -- the
//         members walk; the bytes are known: the whole buffer
//   (ii)  the tail line: every lane reads 2 x 16 B at the head of its own random 128-byte line, 55 of 64 lanes active
//   (iii) the tail block: one 3 200-byte block (100 slots of 32 B) per wave, 55 lanes read 2 x 16 B at block + 32 u for 55 distinct
//         random u of 100
// Prints, per pattern, the time, the lines touched and GB/s of touched lines.  Under `rocprofv3 --pmc FETCH_SIZE` (counters only; give
// `1` as the argument: one launch per pattern) the counter per kernel / lines touched tells what a line of (ii) and (iii) costs
// relative to (i).        hipcc --offload-arch=gfx950 -O3 tools/line_probe.hip -o tools/line_probe
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

typedef float v4f __attribute__((ext_vector_type(4)));
constexpr int NT = 2;                                  // the non-temporal bit of the cache policy
constexpr unsigned LOG_BYTES = 30, BYTES = 1u << LOG_BYTES, LINES = BYTES / 128, ROWS = BYTES / 512, BLOCKS = BYTES / 3200;
constexpr unsigned ODD = 0x9E3779B1u;                  // an odd multiplier: a permutation of any power-of-two range
constexpr unsigned long long PRIME = 2654435761ull;    // coprime to BLOCKS: idx * PRIME % BLOCKS is a permutation

__device__ __forceinline__ v4f ld(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, int soff)
{
    return __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)voff, soff, NT));
}
__device__ __forceinline__ float sum4(v4f a) { return (a.x + a.y) + (a.z + a.w); }

__global__ void __launch_bounds__(256) k_whole_lines(const float *buf, float *out)
{
    __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(buf), 0, (int)BYTES, 0x00020000);
    const unsigned gid = blockIdx.x * blockDim.x + threadIdx.x, cl = gid >> 3, j = gid & 7u, ncl = (gridDim.x * blockDim.x) >> 3;
    float acc = 0.0f;
    for (unsigned r = cl; r < ROWS; r += ncl) {
        const unsigned voff = ((r * ODD) & (ROWS - 1)) * 512u + j * 16u;          // < BYTES
        const v4f a = ld(rsrc, voff, 0), b = ld(rsrc, voff, 128), c = ld(rsrc, voff, 256), d = ld(rsrc, voff, 384);
        acc += (sum4(a) + sum4(b)) + (sum4(c) + sum4(d));
    }
    out[gid] = acc;
}

__global__ void __launch_bounds__(256) k_tail_lines(const float *buf, float *out)
{
    __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(buf), 0, (int)BYTES, 0x00020000);
    const unsigned gid = blockIdx.x * blockDim.x + threadIdx.x, wave = gid >> 6, lane = gid & 63u, nw = (gridDim.x * blockDim.x) >> 6;
    float acc = 0.0f;
    if (lane < 55u) {
        const unsigned step = nw * 55u;
        for (unsigned i = wave * 55u + lane; i < LINES; i += 4u * step) {          // four lines per turn: eight loads in flight
            v4f a[4], b[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const unsigned ik = i + (unsigned)k * step;
                const unsigned voff = ik < LINES ? ((ik * ODD) & (LINES - 1)) * 128u : 0x7ffffff0u;      // (beyond the last line: out of range, zeros, no memory touched)
                a[k] = ld(rsrc, voff, 0); b[k] = ld(rsrc, voff, 16);
            }
#pragma unroll
            for (int k = 0; k < 4; k++) acc += sum4(a[k]) + sum4(b[k]);
        }
    }
    out[gid] = acc;
}

// the slot of lane l in the block with number `blk`: 55 distinct u of 100 (a unit of Z/100 times l, shifted)
__host__ __device__ inline unsigned slot_of(unsigned blk, unsigned l)
{
    const unsigned units[8] = {1u, 3u, 7u, 9u, 11u, 13u, 17u, 19u};
    const unsigned h = blk * ODD;
    return (units[(h >> 28) & 7u] * l + (h >> 8)) % 100u;
}

__global__ void __launch_bounds__(256) k_tail_block(const float *buf, float *out)
{
    __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(buf), 0, (int)BYTES, 0x00020000);
    const unsigned gid = blockIdx.x * blockDim.x + threadIdx.x, wave = gid >> 6, lane = gid & 63u, nw = (gridDim.x * blockDim.x) >> 6;
    float acc = 0.0f;
    if (lane < 55u) {
        for (unsigned i = wave; i < BLOCKS; i += 4u * nw) {
            v4f a[4], b[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const unsigned ik = i + (unsigned)k * nw;
                const unsigned blk = (unsigned)((unsigned long long)ik * PRIME % BLOCKS);
                const unsigned voff = ik < BLOCKS ? blk * 3200u + slot_of(blk, lane) * 32u : 0x7ffffff0u;   // (BLOCKS * 3200 <= BYTES)
                a[k] = ld(rsrc, voff, 0); b[k] = ld(rsrc, voff, 16);
            }
#pragma unroll
            for (int k = 0; k < 4; k++) acc += sum4(a[k]) + sum4(b[k]);
        }
    }
    out[gid] = acc;
}

int main(int argc, char **argv)
{
    const int reps = argc > 1 ? atoi(argv[1]) : 6;
    const unsigned grid = 256 * 8, block = 256;              // 8 workgroups of 4 waves per CU: every wave slot a kernel of this size gets
    float *buf, *out;
    CK(hipMalloc(&buf, (size_t)BYTES));
    CK(hipMemset(buf, 0, (size_t)BYTES));
    CK(hipMalloc(&out, (size_t)grid * block * 4));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    // the lines pattern (iii) touches, counted on the host from the same arithmetic
    unsigned long long block_lines = 0;
    for (unsigned blk = 0; blk < BLOCKS; blk++) {
        unsigned m = 0;                                       // 25 lines of 4 slots
        for (unsigned l = 0; l < 55; l++) m |= 1u << (slot_of(blk, l) >> 2);
        block_lines += (unsigned)__builtin_popcount(m);
    }
    struct { const char *name; void (*k)(const float *, float *); double lines, useful; } pat[3] = {
        {"(i)   whole lines, clusters of 8 x 16 B, 4 lines per row", k_whole_lines, (double)LINES, (double)BYTES},
        {"(ii)  32 B at the head of a line of its own, 55 / 64 lanes", k_tail_lines, (double)LINES, (double)LINES * 32.0},
        {"(iii) 32 B slots of a 3200 B block, 55 of 100 per wave", k_tail_block, (double)block_lines, (double)BLOCKS * 55.0 * 32.0}};
    for (auto &p : pat) {
        float best = 1e30f;
        for (int it = 0; it < reps; it++) {
            CK(hipEventRecord(e0, 0));
            hipLaunchKernelGGL(p.k, dim3(grid), dim3(block), 0, 0, buf, out);
            CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1));
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            if ((reps == 1 || it > 0) && ms < best) best = ms;
        }
        CK(hipGetLastError());
        printf("%-62s %8.3f ms  lines touched %10.0f  (%.2f per block)  useful %7.1f MB  %6.2f TB/s of touched lines  %6.1f ns per 1000 lines\n", p.name, best, p.lines,
               p.lines / BLOCKS, p.useful / 1e6, p.lines * 128.0 / (best * 1e-3) / 1e12, best * 1e6 / (p.lines / 1000.0));
    }
    return 0;
}
