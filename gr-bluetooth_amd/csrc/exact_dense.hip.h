// exact_dense.hip.h -- exact rows, dense form: CHANNELS are the matrix rows, the decimation D is a run-time argument.
//
// exact.hip.h's kernel takes one (channel, tile) pair at a time with the 14 tap blocks as the rows of v_mfma_f32_32x32x2_f32:
// 28 of 32 rows, one trip of the partial sums G through LDS, one barrier and one epilogue per channel, and one instantiation per
// D (its B operand is a register array).  It wins where presence marks a few channels per tile.  Where (nearly) every channel
// is marked -- BTGPU_FLAG_EXACT_ALL -- and at the decimations it is not instantiated for, this form runs:
//
//     M = (channel, re / im): 16 channels per 32-row block (79 channels: 158 of 160 rows)
//     N = output instants: wave w owns the tile's columns [32 w, 32 w + 32)
//     K = the 2 D floats of ONE tap block q;  the accumulator starts at +0 for every q
//
// SUMMATION ORDER -- exact.hip.h's, i.e. the oracle's: inside a tap block the matrix instruction's chain IS the fmaf chain over r
// ascending from +0 (re: fmaf(tr, xr, .) then fmaf(-ti, xi, .)); the blocks' results are added on the vector ALU, y = G[0], then
// y = y + G[q] for q ascending.  Only the 32x32x2 instruction is used: it is the one whose chain was checked on the device.
//
// B (the input): the tile's 128 D samples are staged ONCE per tile into LDS with coalesced loads (int16 widened there), column by
// column as [column][re | im][r], r padded to whole 16-byte groups: for tap block q and four steps the lane of column n, half
// kh reads ONE 16-byte word of column n + q.  The column stride is 2 dpad + 4 floats: (stride / 4) is odd, so the 16 columns of a
// quarter-wave's 16-byte reads cover all 64 banks once.  No register array sized by D: one kernel serves every decimation.
// A (the taps): exact_pack_taps_dense's buffer, a linear stream per wave -- one 16-byte load per lane and four matrix instructions
// (the sparse form's ratio), kept three groups ahead of use in a rotating register copy.
// Epilogue, once per 16 channels: in the C/D layout a lane holds re and im of eight channels of its column.  De-rotation and the
// demodulator run there (y[n - 1] is the neighbouring lane's; across a wave's first column it comes through LDS); the demodulated
// values pass through LDS once -- 1 / 14 of the sparse form's G bytes -- and leave with the lanes remapped: 16 consecutive
// channels of a row of d[g][.] are one 64-byte segment, dcol's runs over g are contiguous.  TWO barriers per row block (the
// wave-boundary y, then the d tile) against the sparse form's one per CHANNEL.
// The stores are masked by the bitmap bit of (tile, channel), a row block with no bit set is skipped: under BTGPU_FLAG_EXACT_ALL
// every bit is set, on the presence path exactly the marked pairs are rewritten -- the sparse form's meaning.
#pragma once
#include "exact.hip.h"

namespace btgpu {

constexpr int kEdDS = kExDenseRows + 1;         // floats per column of the d tile in LDS (odd: the time-major writes and both remapped reads spread over the banks)
constexpr int exact_dense_cs(int D) { return 2 * exact_dpad(D) + 4; }      // floats per staged column
// LDS: the staged tile + the d tile + the waves' last columns + the arctangent table -- 65.6 KB at D = 50 (two workgroups per CU), 9.7 KB at D = 4
inline size_t exact_dense_lds_bytes(int D)
{
    return (size_t)(kExCols * exact_dense_cs(D) + kExCols * kEdDS + kExWaves * 2 * kExDenseRows + 260) * sizeof(float);
}

// FMT: input format (kernels.hip.h); the staging loads single samples (a tile's first sample has either parity), for int8 as
// 16-bit loads that a wave issues over 128 consecutive bytes
template <int FMT>
__device__ __forceinline__ void exact_dense_body(const ExactParams &p, const float2 *__restrict__ x)
{
#pragma clang fp contract(off)
    HIP_DYNAMIC_SHARED(float2, lds)
    const int D = p.D, DP = exact_dpad(D), NI = DP >> 2, CS = exact_dense_cs(D);
    const int rem = D - 4 * (NI - 1);                              // matrix instructions of a tap block's last group: no instruction for a pad step
    float *Bs = (float *)lds;                                      // [kExCols][CS]
    float *Ds = Bs + kExCols * CS;                                 // [kExCols][kEdDS]
    float *Yb = Ds + kExCols * kEdDS;                              // [kExWaves][16 channels][re, im]: y of each wave's LAST column
    float *atab = Yb + kExWaves * 2 * kExDenseRows;
    const int tid = (int)threadIdx.x, lane = tid & 63;
#if defined(__HIP_DEVICE_COMPILE__)
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#else
    const int wave = tid >> 6;
#endif
    const int n = lane & 31, kh = lane >> 5;
    const int u = 32 * wave + n;                                   // this lane's column = output u of the tile (u = 0: the demodulator's halo)
    const int nblk = exact_dense_blocks(p.nch);
    for (int i = tid; i < 257; i += kExThreads) atab[i] = p.atan_tab[i];
    for (int tile = (int)blockIdx.x; tile < p.ntiles; tile += (int)gridDim.x) {
        uint32_t bm[kExWords];
        uint32_t any = 0;
#pragma unroll
        for (int i = 0; i < kExWords; i++) { bm[i] = p.bitmap[(size_t)tile * kExWords + i]; any |= bm[i]; }
        if (!any) continue;                                        // uniform
        if (p.stat && tid == 0) { unsigned int c = 0; for (int i = 0; i < kExWords; i++) c += (unsigned int)__popc(bm[i]); atomicAdd(p.stat, c); }
        const long long g0 = exact_tile_row0(tile) - 1;            // grid row of output 0
        const int nout = (int)(((tile + 1) % kExSlotTiles == 0 ? (long long)(tile / kExSlotTiles + 1) * kExSlotRows : exact_tile_row0(tile + 1)) - g0);   // outputs incl. the halo (115, or 111 for a slot's last)
        const long long sb = p.first0 + g0 * D;                    // the tile's first sample
        __syncthreads();                                           // (the previous tile's matrix instructions have read Bs, its stores Ds)
        // ---- B: sample s of the tile = (column s / D, step s % D); consecutive lanes take consecutive samples ----
        {
            const int total = kExCols * D, dm = kExThreads / D, dr = kExThreads - dm * D;
            int m = tid / D, r = tid - m * D;
            const bool inside = sb >= 0 && sb + total <= p.x_len;  // uniform
            for (int s = tid; s < total; s += kExThreads) {
                float2 v;
                if (inside) v = load_sample<FMT>(x, sb + s);
                else {
                    const long long a = sb + s;
                    v = load_sample<FMT>(x, a < 0 ? 0 : (a < p.x_len ? a : p.x_len - 1));
                    if (!(a >= 0 && a < p.x_len)) v = make_float2(0.f, 0.f);
                }
                Bs[m * CS + r] = v.x;
                Bs[m * CS + DP + r] = v.y;
                m += dm; r += dr;
                if (r >= D) { r -= D; m++; }
            }
        }
        __syncthreads();
        const long long g = g0 + u;
        const bool row_ok = u >= 1 && u < nout && g >= 1 && g < p.G;
        const unsigned int gq = (unsigned int)(g > 0 ? g : 0);
        const unsigned int rot_i = gq % (unsigned int)p.Qr;
        const float *bp = Bs + kh * DP;
        for (int b = 0; b < nblk; b++) {
            const uint32_t bw = b < 2 ? bm[0] : (b < 4 ? bm[1] : bm[2]);                 // (static indices: a run-time one puts bm in scratch memory)
            const uint32_t mask = (bw >> (16 * (b & 1))) & 0xffffu;                      // the bitmap bits of this block's 16 channels
            if (!mask) continue;                                   // uniform
            // ---- the 14 tap blocks ----
            const float4 *ap = (const float4 *)p.tapsD + (size_t)b * kExQB * NI * 64 + lane;
            float4 a0 = ap[0], a1 = ap[64], a2 = ap[128];
            ap += 192;
            float4 bn = *(const float4 *)(bp + u * CS);
            f32x16 y;
            for (int q = 0; q < kExQB; q++) {
                // column n + q of the tile; the columns past 127 belong to outputs >= 115, which no tile keeps
                const float *bq = bp + (u + q < kExCols ? u + q : kExCols - 1) * CS;
                const float *bq1 = bp + (u + q + 1 < kExCols ? u + q + 1 : kExCols - 1) * CS;
                f32x16 acc;
#pragma unroll
                for (int i = 0; i < 16; i++) acc[i] = 0.f;
                for (int i = 0; i < NI - 1; i++) {
                    const float4 a = a0, bv = bn;
                    a0 = a1; a1 = a2; a2 = *ap; ap += 64;
                    bn = *(const float4 *)(bq + 4 * (i + 1));
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bv.x, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bv.y, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bv.z, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bv.w, acc, 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);             // (keep the loads HERE, ahead of their use: exact.hip.h)
                }
                {
                    const float4 a = a0, bv = bn;
                    a0 = a1; a1 = a2; a2 = *ap; ap += 64;          // (behind the block's last group: the next block's, or the zero groups)
                    bn = *(const float4 *)bq1;                     // the next tap block's first group (q = 13: read, unused)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bv.x, acc, 0, 0, 0);
                    if (rem > 1) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bv.y, acc, 0, 0, 0);
                    if (rem > 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bv.z, acc, 0, 0, 0);
                    if (rem > 3) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bv.w, acc, 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (q == 0) y = acc;
                else {
#pragma unroll
                    for (int i = 0; i < 16; i++) y[i] = y[i] + acc[i];
                }
            }
            // ---- epilogue of the block's 16 channels.  C/D layout: register 4 j + e = row 8 j + 4 kh + e of column n, i.e. for
            // k = 2 j + h the lane holds channel cl = 4 j + 2 kh + h of the block: re in register 4 j + 2 h, im in the next ----
            float2 yv[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int cl = 4 * (k >> 1) + 2 * kh + (k & 1), c = kExDenseRows * b + cl;
                const float2 rt = p.rot[(size_t)(c < p.nch ? c : p.nch - 1) * p.Qr + rot_i];
                const float yr = y[4 * (k >> 1) + 2 * (k & 1)], yi = y[4 * (k >> 1) + 2 * (k & 1) + 1];
                yv[k].x = fmaf(-yi, rt.y, yr * rt.x);
                yv[k].y = fmaf(yi, rt.x, yr * rt.y);
                if (p.ydbg && c < p.nch && ((mask >> cl) & 1u) && u < nout && g >= 0 && g < p.G) p.ydbg[(size_t)c * p.ystride + g] = yv[k];
                if (n == 31) { Yb[(wave * kExDenseRows + cl) * 2] = yv[k].x; Yb[(wave * kExDenseRows + cl) * 2 + 1] = yv[k].y; }
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int cl = 4 * (k >> 1) + 2 * kh + (k & 1);
                float2 yp;                                         // y[u - 1]: the left neighbour's; of a wave's first column: the wave before's last
                yp.x = __shfl_up(yv[k].x, 1, 64); yp.y = __shfl_up(yv[k].y, 1, 64);
                if (n == 0 && wave > 0) { yp.x = Yb[((wave - 1) * kExDenseRows + cl) * 2]; yp.y = Yb[((wave - 1) * kExDenseRows + cl) * 2 + 1]; }
                Ds[u * kEdDS + cl] = row_ok ? demod_one(atab, p.gain, yv[k], yp) : 0.f;      // (u = 0 has no neighbour and is no row: row_ok)
            }
            __syncthreads();
            // ---- stores, lanes remapped.  d[g][.]: 16 lanes = the block's 16 channels of one row ----
            if (p.d) {
                const int cl = tid & 15, c = kExDenseRows * b + cl;
                const bool c_ok = c < p.nch && ((mask >> cl) & 1u);
#pragma unroll
                for (int k = 0; k < kExCols / 16; k++) {
                    const int u2 = (tid >> 4) + 16 * k;
                    const long long g2 = g0 + u2;
                    if (c_ok && u2 >= 1 && u2 < nout && g2 >= 1 && g2 < p.G) p.d[(size_t)g2 * p.drow + c] = Ds[u2 * kEdDS + cl];
                }
            }
            if (p.dcol) {                                          // [G / 25][80][25]: consecutive lanes = consecutive rows of one channel
                const int u2 = tid & (kExCols - 1);
                const long long g2 = g0 + u2;
                const bool g_ok = u2 >= 1 && u2 < nout && g2 >= 1 && g2 < p.G;
                const unsigned int gu = (unsigned int)(g2 > 0 ? g2 : 0);
                float *dc = p.dcol + (size_t)(gu / 25u) * (80u * 25u) + gu % 25u;
#pragma unroll
                for (int k = 0; k < kExDenseRows / 2; k++) {
                    const int cl = (tid >> 7) + 2 * k, c = kExDenseRows * b + cl;
                    if (g_ok && c < p.nch && ((mask >> cl) & 1u)) dc[25 * c] = Ds[u2 * kEdDS + cl];
                }
            }
        }
    }
}

__global__ __launch_bounds__(kExThreads, 2) void exact_dense_kernel(ExactParams p, const float2 *__restrict__ x)
{
    exact_dense_body<kInF32>(p, x);
}
// (a template only so that it can be instantiated in the int16 kernels' translation unit: s16_inst.h)
template <int V = 0>
__global__ __launch_bounds__(kExThreads, 2) void exact_dense_kernel_s16(ExactParams p, const float2 *__restrict__ x)
{
    exact_dense_body<kInS16>(p, x);
}
template <int V = 0>
__global__ __launch_bounds__(kExThreads, 2) void exact_dense_kernel_s8(ExactParams p, const float2 *__restrict__ x)
{
    exact_dense_body<kInS8>(p, x);
}

}  // namespace btgpu
