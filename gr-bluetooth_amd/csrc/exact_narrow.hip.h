// exact_narrow.hip.h -- exact rows, narrow form: EIGHT channels x (re, im) are the 16 rows of v_mfma_f32_16x16x4_f32.
//
// For the handles with few channels (decimation D <= 8: the even rates 4 .. 16 Msps, 1 or 2 row blocks of eight channels).  There
// exact.hip.h's kernel issues D matrix instructions per (channel, tile) and then sends 16 KB of partial sums through LDS behind a
// barrier, and exact_dense.hip.h's 32-row blocks stand half empty.  This form's matrix shape fits those handles:
//
//     M = (channel, re / im): row 2 cl + (re: 0, im: 1) of channel 8 b + cl; row block b = blockIdx.y
//     N = 16 output instants: a wave owns TWO column groups (independent accumulators, their instructions interleave: a dependent
//         chain loses its forwarding, exact.hip.h F12); group j = 2 wave + h holds the tile's outputs 15 j .. 15 j + 15
//     K = the 2 D interleaved floats of ONE tap block q, padded to whole instructions of 4; the accumulator starts at +0 for every q
//
// no idle row, no partial sums in LDS, no barrier behind the staging, and the row block's whole tap set -- 14 blocks x ceil(2 D / 4)
// instructions, one float per lane each: <= 56 VGPRs -- loaded ONCE per workgroup, which strides over the tiles.
//
// SUMMATION ORDER -- exact.hip.h's, i.e. the oracle's: inside a tap block the fmaf chain over the interleaved floats ascending from
// +0 (re: fmaf(tr, xr, .) then fmaf(-ti, xi, .)), which v_mfma_f32_16x16x4_f32 is bit for bit, k = 0, 1, 2, 3 of instruction 0, then
// of instruction 1 ... (scripts/ubench/exact_mfma.hip mfma16, profiles/ubench_mfma_16x16x4.txt: 5.2e9 products, 0 outputs differ);
// the blocks' results are added on the vector ALU, y = G[0], then y = y + G[q] for q ascending.
// THE K PAD (odd D): zero taps against zero staged input.  A block's chain starts at +0 and a sum that rounds to zero is +0 in
// round-to-nearest, so the accumulator is never -0: a padded step, acc + (+0), leaves it unchanged.
//
// B (the input): the tile's 128 columns of D samples are staged once per tile into LDS with coalesced loads through load_sample<FMT>.
// Inside a column the floats are permuted to [k][i], i = the matrix instruction, k = its step: what the lane of column n, step k
// needs for ALL instructions of a tap block is ONE 4-, 8- or 16-byte read of column n + q (NI = 1, 2, 3 .. 4).
// COLUMN PITCH (narrow_pitch): 4 NIP floats of data + 4 floats of pad where NIP > 1.
//     NIP = 4 (pitch 20): a 16-byte read is served 16 lanes at a time -- one k, columns n .. n + 15 at 16-byte word 5 n + k: 5 is
//         odd, the 16 words fall into the 16 different four-bank groups;
//     NIP = 2 (pitch 12): an 8-byte read 32 lanes at a time -- k = 0, 1 (or 2, 3), 8-byte word 6 n + k: 6 n mod 32 takes 16
//         different even values (3 is odd), + k fills the odd ones: all 32 bank pairs once;
//     NIP = 1 (pitch 4): the 64 lanes read floats 4 n + k, the 64 banks once.
// Six zero columns behind the tile's 128 take the reads of the outputs past 114 (column u + q <= 133), which no tile keeps.
// Epilogue in the C/D layout: register e = row 4 k + e of column n, i.e. the lane holds re and im of channels 2 k and 2 k + 1 of
// its column.  Each group's column 0 is the output BEFORE its first row (the demodulator's halo), so y[n - 1] is always the lane to
// the left in the same 16-lane row: one DPP move, nothing crosses a group or a wave.  De-rotation and demod_one as in exact.hip.h;
// the two demodulated values leave as one 8-byte store into the time-major stream (eight channels of a row = one 32-byte
// sector), masked by the bitmap bits; a row block without a bit is skipped before staging.
// (No tile-blocked stream: that one belongs to the 100-bin bank, D = 50.)
#pragma once
#include "exact.hip.h"

namespace btgpu {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kEnRows = 8;                                       // channels per 16-row block
constexpr int kEnMaxD = 8;
constexpr int kEnCols = kExCols + 6;                             // staged columns + the zero columns (output 120, tap block 13)
constexpr int kEnWgPerCu = 4, kEnGridX = 256 * kEnWgPerCu;       // workgroups striding over the tiles: four on each of 256 CUs
static_assert(2 * kExWaves * 15 >= kExTile, "the column groups hold a tile's rows");
static_assert(15 * (2 * kExWaves - 1) + 15 + kExQB - 1 < kEnCols, "every read of the tap blocks stays inside the staged columns");
constexpr int narrow_ni(int D) { return (2 * D + 3) / 4; }       // matrix instructions per tap block
constexpr int narrow_nip(int NI) { return NI == 3 ? 4 : NI; }    // floats per (column, k): one 4-, 8- or 16-byte read
constexpr int narrow_pitch(int NI) { return 4 * narrow_nip(NI) + (NI > 1 ? 4 : 0); }
constexpr int exact_narrow_blocks(int nch) { return (nch + kEnRows - 1) / kEnRows; }
// LDS: the staged tile + the arctangent table -- 7.5 KB at D = 4, 11.8 KB at D = 8
inline size_t exact_narrow_lds_bytes(int D) { return (size_t)(kEnCols * narrow_pitch(narrow_ni(D)) + 260) * sizeof(float); }

template <int NI, int FMT>
__device__ __forceinline__ void exact_narrow_body(const ExactParams &p, const float2 *__restrict__ x)
{
#pragma clang fp contract(off)
    HIP_DYNAMIC_SHARED(float2, lds)
    constexpr int NIP = narrow_nip(NI), CP = narrow_pitch(NI);
    float *Bs = (float *)lds;                                      // [kEnCols][CP]
    float *atab = Bs + kEnCols * CP;
    const int D = p.D;
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 15, kh = lane >> 4, b = (int)blockIdx.y;
    // ---- A: the row block's 14 tap blocks, once per workgroup (exact_pack_taps_narrow: [b][q][i][lane]) ----
    float A[kExQB][NI];
    {
        const float *ap = p.tapsD + (size_t)b * kExQB * NI * 64 + lane;
#pragma unroll
        for (int q = 0; q < kExQB; q++)
#pragma unroll
            for (int i = 0; i < NI; i++) A[q][i] = ap[(q * NI + i) * 64];
    }
    for (int i = tid; i < 257; i += kExThreads) atab[i] = p.atan_tab[i];
    for (int i = tid; i < kEnCols * CP; i += kExThreads) Bs[i] = 0.f;    // the K pad and the zero columns: never written again
    const int c0 = kEnRows * b + 2 * kh;                           // this lane's two channels: c0, c0 + 1
    const float2 *rot0 = p.rot + (size_t)(c0 < p.nch ? c0 : p.nch - 1) * p.Qr;
    const float2 *rot1 = p.rot + (size_t)(c0 + 1 < p.nch ? c0 + 1 : p.nch - 1) * p.Qr;
    for (int tile = (int)blockIdx.x; tile < p.ntiles; tile += (int)gridDim.x) {
        const uint32_t mask = (p.bitmap[(size_t)tile * kExWords + (b >> 2)] >> (8 * (b & 3))) & 0xffu;   // the bitmap bits of this block's 8 channels
        if (!mask) continue;                                       // uniform
        if (p.stat && tid == 0) atomicAdd(p.stat, (unsigned int)__popc(mask));
        const long long g0 = exact_tile_row0(tile) - 1;            // grid row of output 0
        const int nout = (int)(((tile + 1) % kExSlotTiles == 0 ? (long long)(tile / kExSlotTiles + 1) * kExSlotRows : exact_tile_row0(tile + 1)) - g0);   // outputs incl. the halo (115, or 111 for a slot's last)
        const long long sb = p.first0 + g0 * D;                    // the tile's first sample
        __syncthreads();                                           // (the previous tile's reads of Bs; the first tile: the zeros)
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
                // float f = 2 r (re), 2 r + 1 (im) of the column = step k = f & 3 of instruction i = f >> 2, at [k][i]
                float *bw = Bs + m * CP + 2 * (r & 1) * NIP + (r >> 1);
                bw[0] = v.x;
                bw[NIP] = v.y;
                m += dm; r += dr;
                if (r >= D) { r -= D; m++; }
            }
        }
        __syncthreads();
        // ---- the 14 tap blocks of the wave's two column groups ----
        const int u0 = 15 * (2 * wave) + n, u1 = u0 + 15;          // this lane's columns = outputs u0, u1 of the tile (n = 0: the group's halo)
        const float *bp0 = Bs + u0 * CP + kh * NIP, *bp1 = bp0 + 15 * CP;
        auto read_b = [&](const float *bp, float (&o)[4]) {        // column u + q, this lane's step of every instruction: one read
            if constexpr (NIP == 1) o[0] = bp[0];
            else if constexpr (NIP == 2) { const float2 t = *(const float2 *)bp; o[0] = t.x; o[1] = t.y; }
            else { const float4 t = *(const float4 *)bp; o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w; }
        };
        // Software pipeline: block q's two chains, with the reads of block q + 1 ahead of them and the vector adds of block q - 1
        // behind them.  Left alone the compiler issues all 28 chains at once -- 112 accumulator registers, the taps in scratch
        // memory -- and a sched_barrier does not hold the adds, which have no side effect: the empty asm at the end of a block
        // takes y and the next block's B through it, so that block q + 1's chains follow block q - 1's adds.
        // The ORDER of the adds is untouched: y = G[0], then + G[1], ...
        float bn0[4], bn1[4];
        read_b(bp0, bn0); read_b(bp1, bn1);
        f32x4 y0 = {0.f, 0.f, 0.f, 0.f}, y1 = y0, g0v = y0, g1v = y0;
#pragma unroll
        for (int q = 0; q < kExQB; q++) {
            float b0[4], b1[4];
#pragma unroll
            for (int i = 0; i < NIP; i++) { b0[i] = bn0[i]; b1[i] = bn1[i]; }
            if (q + 1 < kExQB) { read_b(bp0 + (q + 1) * CP, bn0); read_b(bp1 + (q + 1) * CP, bn1); }
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < NI; i++) {
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(A[q][i], b0[i], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(A[q][i], b1[i], acc1, 0, 0, 0);
            }
            if (q == 1) { y0 = g0v; y1 = g1v; }
            else if (q > 1) {
#pragma unroll
                for (int e = 0; e < 4; e++) { y0[e] = y0[e] + g0v[e]; y1[e] = y1[e] + g1v[e]; }
            }
            g0v = acc0; g1v = acc1;
            if constexpr (NIP == 1) asm volatile("" : "+v"(y0), "+v"(y1), "+v"(bn0[0]), "+v"(bn1[0]));
            else if constexpr (NIP == 2) asm volatile("" : "+v"(y0), "+v"(y1), "+v"(bn0[0]), "+v"(bn0[1]), "+v"(bn1[0]), "+v"(bn1[1]));
            else asm volatile("" : "+v"(y0), "+v"(y1), "+v"(bn0[0]), "+v"(bn0[1]), "+v"(bn0[2]), "+v"(bn0[3]), "+v"(bn1[0]), "+v"(bn1[1]), "+v"(bn1[2]), "+v"(bn1[3]));
        }
#pragma unroll
        for (int e = 0; e < 4; e++) { y0[e] = y0[e] + g0v[e]; y1[e] = y1[e] + g1v[e]; }
        // ---- epilogue: registers (0, 1) = (re, im) of channel c0, (2, 3) of c0 + 1, at this lane's column ----
        const bool ok0 = c0 < p.nch && ((mask >> (2 * kh)) & 1u), ok1 = c0 + 1 < p.nch && ((mask >> (2 * kh + 1)) & 1u);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const f32x4 y = h ? y1 : y0;
            const int u = h ? u1 : u0;
            const long long g = g0 + u;
            const bool row_ok = n >= 1 && u < nout && g >= 1 && g < p.G;     // (n = 0 has no neighbour and is the row of the group before)
            const unsigned int gq = (unsigned int)(g > 0 ? g : 0);
            const unsigned int rot_i = gq % (unsigned int)p.Qr;
            float dv[2];
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const float2 rt = (k ? rot1 : rot0)[rot_i];
                const float yr = y[2 * k], yi = y[2 * k + 1];
                float2 yv, yp;
                yv.x = fmaf(-yi, rt.y, yr * rt.x);
                yv.y = fmaf(yi, rt.x, yr * rt.y);
                // y[u - 1]: the lane to the left in this row of 16 lanes (row_shr:1)
                yp.x = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(yv.x), 0x111, 0xf, 0xf, false));
                yp.y = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(yv.y), 0x111, 0xf, 0xf, false));
                dv[k] = demod_one(atab, p.gain, yv, yp);
            }
            if (row_ok) {
                float *dp = p.d + (size_t)gq * p.drow + c0;        // (win_drow is even, c0 is: 8-byte aligned)
                if (ok0 && ok1) *(float2 *)dp = make_float2(dv[0], dv[1]);
                else if (ok0) dp[0] = dv[0];
                else if (ok1) dp[1] = dv[1];
            }
        }
    }
}

// one kernel per number of matrix instructions in a tap block: NI = 1 (D = 2), 2 (D = 3, 4), 3 (D = 5, 6), 4 (D = 7, 8)
template <int NI>
__global__ __launch_bounds__(kExThreads, kEnWgPerCu) void exact_narrow_kernel(ExactParams p, const float2 *__restrict__ x)
{
    exact_narrow_body<NI, kInF32>(p, x);
}
template <int NI>
__global__ __launch_bounds__(kExThreads, kEnWgPerCu) void exact_narrow_kernel_s16(ExactParams p, const float2 *__restrict__ x)
{
    exact_narrow_body<NI, kInS16>(p, x);
}
template <int NI>
__global__ __launch_bounds__(kExThreads, kEnWgPerCu) void exact_narrow_kernel_s8(ExactParams p, const float2 *__restrict__ x)
{
    exact_narrow_body<NI, kInS8>(p, x);
}

template <int FMT = kInF32>
inline ExactRowsKernel exact_narrow_pick(int D)
{
    if (D < 2 || D > kEnMaxD) return nullptr;
    switch (narrow_ni(D)) {
#define BTGPU_EN(n) case n: if constexpr (FMT == kInS8) return exact_narrow_kernel_s8<n>; else if constexpr (FMT == kInS16) return exact_narrow_kernel_s16<n>; else return exact_narrow_kernel<n>;
        BTGPU_EN(1) BTGPU_EN(2) BTGPU_EN(3) BTGPU_EN(4)
#undef BTGPU_EN
    }
    return nullptr;
}

}  // namespace btgpu
