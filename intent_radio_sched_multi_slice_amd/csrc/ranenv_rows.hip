// ranenv_rows.hip -- the PPO row lists on the device (ranenv_ppo_row_count / ranenv_ppo_row_order; include/ranenv.h "Row lists on the
// device"): a stable compaction of the live intra cells of a record, grouped by member or by slice, and per epoch and unit a keyed
// permutation of the unit's rows, computed per entry.  Four kernels under the spread binding's rules: no atomics, no barrier across
// workgroups, no flags -- what a launch writes, only later launches read, so the lists are a function of the inputs alone.
#include "ranenv_numeric.hpp"

namespace {

constexpr int ROWS_BLOCK = 256, ROWS_WAVES = ROWS_BLOCK / WAVE, ROWS_PER_WAVE = ROWS_CHUNK / ROWS_WAVES / WAVE;      // 4 waves, 8 rows of 64 cells each
constexpr unsigned ROWS_TAG = 0x53485546u;              // "SHUF": counter word c3 of the keys' Philox blocks, + block

// Chunk `g` of the geometry: its unit, and its cells as first + i * stride for 0 <= i < len
struct RowsChunk { int unit; long long first; int stride, len; };
DEVFN RowsChunk rows_chunk(const RowsGeom &G, int g)
{
    int u = 0;
    for (int m = 1; m < G.units; m++) u += g >= G.chunk_first[m] ? 1 : 0;      // (uniform: the table is read with scalar loads)
    int c0 = 0, per = 1, e0 = 0, e1 = 0;
    for (int m = 0; m < G.units; m++)
        if (m == u) { c0 = G.chunk_first[m]; per = G.chunks_per[m]; e0 = G.first_env[m]; e1 = G.first_env[m + 1]; }
    const int c = g - c0;
    RowsChunk k;
    k.unit = u;
    if (G.grouping == RANENV_PPO_ROWS_SLICES) {         // a run of record rows t * B + b at the fixed slice u
        const long long r0 = (long long)c * ROWS_CHUNK, rows = (long long)G.T * G.B;
        k.first = r0 * G.S + u; k.stride = G.S;
        k.len = (int)(rows - r0 < ROWS_CHUNK ? rows - r0 : ROWS_CHUNK);
    } else {                                            // a piece of the member's env range at one TTI: contiguous in [t][b][s]
        const int t = c / per, j = c - t * per;
        const long long seg = (long long)(e1 - e0) * G.S, o = (long long)j * ROWS_CHUNK;
        k.first = ((long long)t * G.B + e0) * G.S + o; k.stride = 1;
        k.len = (int)(seg - o < ROWS_CHUNK ? seg - o : ROWS_CHUNK);
    }
    return k;
}

// The live cells of a chunk as the wave sees them: wave w owns cells [w * 512, (w + 1) * 512) of the chunk in 8 rows of 64, lane l
// cell w * 512 + q * 64 + l of row q; bit l of live[q] says that cell is inside the chunk and its mask byte is not 0
DEVFN int rows_ballots(const int8_t *mask, const RowsChunk &k, int wave, int lane, unsigned long long (&live)[ROWS_PER_WAVE])
{
    int total = 0;
#pragma unroll
    for (int q = 0; q < ROWS_PER_WAVE; q++) {
        const int i = (wave * ROWS_PER_WAVE + q) * WAVE + lane;
        const bool on = i < k.len && mask[k.first + (long long)i * k.stride] != 0;
        live[q] = __ballot(on);
        total += __popcll(live[q]);
    }
    return total;
}

// COUNT: one workgroup per chunk, its live cells into counts[chunk]
__global__ void __launch_bounds__(ROWS_BLOCK) ranenv_rows_count_kernel(RowsGeom G, const int8_t *mask, int32_t *counts)
{
    __shared__ int wave_total[ROWS_WAVES];
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const RowsChunk k = rows_chunk(G, blockIdx.x);
    unsigned long long live[ROWS_PER_WAVE];
    const int total = rows_ballots(mask, k, wave, lane, live);
    if (lane == 0) wave_total[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
        for (int w = 0; w < ROWS_WAVES; w++) n += wave_total[w];
        counts[blockIdx.x] = n;
    }
}

// SCAN: one workgroup, the exclusive prefix of counts[0 .. n_chunks) into offsets (the chunks are numbered unit-major, so chunk g's
// offset is its unit's `first` entry plus the live cells of the unit's chunks before it), and the units' table first[0 .. units]
__global__ void __launch_bounds__(ROWS_BLOCK) ranenv_rows_scan_kernel(RowsGeom G, const int32_t *counts, int32_t *offsets, int32_t *first)
{
    __shared__ int part[ROWS_BLOCK];
    const long long per = ((long long)G.n_chunks + ROWS_BLOCK - 1) / ROWS_BLOCK, lo64 = (long long)threadIdx.x * per;
    const int lo = (int)(lo64 < G.n_chunks ? lo64 : G.n_chunks);
    const int hi = (int)(lo + per < G.n_chunks ? lo + per : G.n_chunks);
    int sum = 0;
    for (int g = lo; g < hi; g++) sum += counts[g];
    part[threadIdx.x] = sum;
    __syncthreads();
    int run = 0;
    for (int t = 0; t < (int)threadIdx.x; t++) run += part[t];
    for (int g = lo; g < hi; g++) {
        for (int m = 0; m < G.units; m++)
            if (G.chunk_first[m] == g) first[m] = run;      // (a unit has at least one chunk: no two units start at one chunk)
        offsets[g] = run;
        run += counts[g];
    }
    if (threadIdx.x == ROWS_BLOCK - 1) first[G.units] = run;      // (the last thread's range ends at n_chunks or is empty behind it)
}

// COMPACT: the count kernel's geometry again; the live cells' numbers into base[offsets[chunk] + rank], rank ascending with the cell.
// n_base: the live cells the count found -- a mask that changed under the two launches' feet writes nothing beyond them
__global__ void __launch_bounds__(ROWS_BLOCK) ranenv_rows_compact_kernel(RowsGeom G, const int8_t *mask, const int32_t *offsets, int32_t *base,
                                                                         long long n_base)
{
    __shared__ int wave_total[ROWS_WAVES];
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const RowsChunk k = rows_chunk(G, blockIdx.x);
    unsigned long long live[ROWS_PER_WAVE];
    const int total = rows_ballots(mask, k, wave, lane, live);
    if (lane == 0) wave_total[wave] = total;
    __syncthreads();
    long long at = offsets[blockIdx.x];
    for (int w = 0; w < wave; w++) at += wave_total[w];
#pragma unroll
    for (int q = 0; q < ROWS_PER_WAVE; q++) {
        const unsigned long long b = live[q];
        const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
        if (((b >> lane) & 1ull) && at + rank < n_base) {
            const int i = (wave * ROWS_PER_WAVE + q) * WAVE + lane;
            base[at + rank] = (int32_t)(k.first + (long long)i * k.stride);
        }
        at += __popcll(b);
    }
}

DEVFN unsigned rows_fmix(unsigned x)
{
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
    return x;
}

// SHUFFLE: one thread per entry (epoch k = blockIdx.y, position p of the epoch's list): its unit u by a walk of the `first` table,
// i = p - first[u], j = P(n_u, seed, k, u, kind)(i), and the j-th row of the unit's base list -- arithmetic for the inter kind, a
// gather from the compacted cells for the intra kind -- into out[k][p]
__global__ void __launch_bounds__(ROWS_BLOCK) ranenv_rows_shuffle_kernel(RowsShuffle A)
{
    const long long p64 = (long long)blockIdx.x * ROWS_BLOCK + threadIdx.x;
    if (p64 >= A.n) return;
    const int p = (int)p64, k = A.k0 + (int)blockIdx.y;
    int u = 0, lo = 0, hi = 1, e0 = 0, e1 = 1;
    for (int m = 0; m < A.units; m++)
        if (p >= A.first[m] && p < A.first[m + 1]) { u = m; lo = A.first[m]; hi = A.first[m + 1]; e0 = A.first_env[m]; e1 = A.first_env[m + 1]; }
    const unsigned n = (unsigned)(hi - lo);
    unsigned x = (unsigned)(p - lo);
    if (n > 1u) {
        unsigned key[8];
        {
            unsigned w[4];
            philox4x32_10((unsigned)k, (unsigned)u, (unsigned)A.kind, ROWS_TAG, (unsigned)A.seed, (unsigned)(A.seed >> 32), w);
            key[0] = w[0]; key[1] = w[1]; key[2] = w[2]; key[3] = w[3];
            philox4x32_10((unsigned)k, (unsigned)u, (unsigned)A.kind, ROWS_TAG + 1u, (unsigned)A.seed, (unsigned)(A.seed >> 32), w);
            key[4] = w[0]; key[5] = w[1]; key[6] = w[2]; key[7] = w[3];
        }
        const int bits = 32 - __clz((int)(n - 1u));     // bit_length(n - 1) >= 1
        const int h = (bits + 1) >> 1;
        const unsigned hm = (1u << h) - 1u;
        do {                                            // (the pass is a bijection of [0, 2^(2h)): the walk comes back into [0, n))
            unsigned L = x >> h, R = x & hm;
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const unsigned nr = L ^ (rows_fmix(R + key[r]) & hm);
                L = R; R = nr;
            }
            x = (L << h) | R;
        } while (x >= n);
    }
    int32_t row;
    if (A.kind == 0) {
        const unsigned bm = (unsigned)(e1 - e0), t = x / bm;
        row = (int32_t)(t * (unsigned)A.B + (unsigned)e0 + (x - t * bm));
    } else {
        row = A.base[(long long)lo + x];
    }
    A.out[(long long)k * A.n + p] = row;
}

}  // namespace

namespace ranenv_dev {

void launch_rows_count(hipStream_t s, const RowsGeom &G, const int8_t *mask, int32_t *counts, int32_t *offsets, int32_t *first)
{
    hipLaunchKernelGGL(ranenv_rows_count_kernel, dim3((unsigned)G.n_chunks), dim3(ROWS_BLOCK), 0, s, G, mask, counts);
    hipLaunchKernelGGL(ranenv_rows_scan_kernel, dim3(1), dim3(ROWS_BLOCK), 0, s, G, counts, offsets, first);
}

void launch_rows_compact(hipStream_t s, const RowsGeom &G, const int8_t *mask, const int32_t *offsets, int32_t *base, long long n_base)
{
    hipLaunchKernelGGL(ranenv_rows_compact_kernel, dim3((unsigned)G.n_chunks), dim3(ROWS_BLOCK), 0, s, G, mask, offsets, base, n_base);
}

void launch_rows_shuffle(hipStream_t s, int epochs, const RowsShuffle &A_)
{
    RowsShuffle A = A_;
    for (int k0 = 0; k0 < epochs; k0 += 65535) {        // (a grid's y extent ends at 65535)
        const int ne = epochs - k0 < 65535 ? epochs - k0 : 65535;
        A.k0 = k0;
        hipLaunchKernelGGL(ranenv_rows_shuffle_kernel, dim3((unsigned)((A.n + ROWS_BLOCK - 1) / ROWS_BLOCK), (unsigned)ne), dim3(ROWS_BLOCK), 0, s, A);
    }
}

}  // namespace ranenv_dev
