// pfbg.hip.h -- polyphase channelizer for the capture rates pfbm.hip.h cannot hold in LDS (M = fs / 1 MHz bins, even: channel bank
// 68..98, squelch stage 1 52..98):
// the algebra, the outputs and the 50-instant tile contract of pfbm.hip.h, with the DFT on the matrix pipe.
//
// Y_c[t] = sum_p u_p[t] W[p][c] written as a real GEMM of K = 2 M with v_mfma_f32_32x32x2_f32:
//     rows    (channel, re / im): wave w of five owns rows [32 w, 32 w + 32) = 16 channels (79 channels: 158 of 160 rows)
//     columns 32 consecutive output instants = one PASS
//     A       the real-ified DFT [[W_re, -W_im], [W_im, W_re]] (pack_dft_rows, design_fast.cc): constant for the launch, loaded
//             ONCE per workgroup with coalesced 16-byte loads and kept in registers -- no DFT table in LDS, the term that put
//             pfbm_kernel over the budget
//     B       the branch outputs U[instant][2 M interleaved floats] in LDS.  The K order is free (the bank is the tolerance path,
//             exact rows repair it): step 4 g + s pairs floats 8 g + s (lanes 0-31) and 8 g + 4 + s (lanes 32-63), so a lane's
//             four consecutive steps are ONE 16-byte read of its row.  Row pitch 8 ng + 4 floats: (pitch / 4) is odd, the 16 rows
//             of a quarter-wave's 16-byte reads cover all 64 banks once.
// A workgroup owns a RUN of consecutive instants (channel bank: whole 50-instant tiles plus ONE halo instant for the demodulator)
// and marches over it in passes, so the halo and the A loads are paid per run, not per tile, and no matrix column is spent on
// padding a 51-instant tile to 64.  Per pass:
//   0  input span of a chunk of instants -> LDS (aligned 16-byte loads, unconditional on interior chunks; int16 widened here)
//   A  lane = (instant, branch): Q taps out of LDS -> U.  Channel bank: one chunk of 32 instants; noise bank (hop 5 D): four
//      chunks of 8, which keeps the staged span under 26 KB at M = 98
//   B  8 ng matrix instructions per wave
//   C  channel bank -- in the C/D layout a lane holds re / im of eight channels at its instant: Y[t - 1] is the neighbouring lane's
//      (the previous pass's last column is kept in registers), demodulate Y[t] conj(Y[t - 1]) rho; angles and |Y|^2 pass through an
//      LDS tile (on top of the dead U) and leave as whole d rows / as the double ptile / phead sums with pfbm's head rule, summed
//      in instant order by one lane per channel -- the same sums whatever the run length.
//      noise bank -- de-rotate with krot, store runs of Z[c][.].
// LDS at M = 98 with float input: 46.5 KB (channel), 63.4 KB (noise).  Registers: 100 hold A, 238 (channel) / 173 (noise) in all, no
// scratch: one workgroup per CU by registers -- bounding the kernel to three waves per SIMD (168) spilled 71 registers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "design.h"
#include "pfbm.hip.h"
#include "exact.hip.h"

namespace btgpu {

constexpr int kPfbgWaves = 5, kPfbgThreads = 64 * kPfbgWaves;
constexpr int kPfbgNG = 25;                   // 16-byte groups of K a lane can hold: 2 M <= 200
constexpr int kPfbgCols = 32;                 // instants per pass
constexpr int kPfbgDS = 16 * kPfbgWaves + 1;  // floats per instant of the angle / |Y|^2 tiles (odd: the time-major writes spread over the banks)
constexpr int kPfbgNoiseRun = 4 * kPfbgCols;  // instants per workgroup of the noise bank

__host__ __device__ inline int pfbg_groups(int M) { return (2 * M + 7) / 8; }
inline int pfbg_chunk(bool chan) { return chan ? kPfbgCols : 8; }
inline bool pfbg_serves(const PfbBank &b, int nch)
{
    return b.available && b.M % 2 == 0 && b.M > 10 && pfbg_groups(b.M) <= kPfbgNG && nch <= 16 * kPfbgWaves;
}
inline size_t pfbg_lds_bytes(int M, int D, int Q, bool chan, bool real)
{
    const int n4 = (D * (pfbg_chunk(chan) - 1) + Q * M + 3) / 2;
    const int taps = ((real ? 1 : 2) * Q * M + 3) & ~3;
    const int u = kPfbgCols * (8 * pfbg_groups(M) + 4), e = chan ? 2 * kPfbgCols * kPfbgDS : 0;
    return (size_t)(4 * n4 + taps + (u > e ? u : e)) * sizeof(float);
}
// tiles per workgroup of the channel bank: long runs where the batch still fills the device with them
inline int pfbg_run_tiles(int ntiles) { return ntiles >= 16 * 1024 ? 16 : ntiles >= 8 * 512 ? 8 : ntiles >= 4 * 256 ? 4 : 2; }

struct PfbgParams {
    PfbmParams m;                // as launch_channel_bank_m / launch_noise_bank_m fill it (TT = 50: the tile sums' grid)
    const float4 *arows;         // pack_dft_rows: [wave][ng][64 lanes] x 4 steps
    int ng;                      // pfbg_groups(M)
    int run;                     // new instants per workgroup (channel bank: a multiple of TT)
};

// FMT: input format of the stream (kernels.hip.h); int8 pieces are aligned 32-bit words from the even sample a0, edge chunks
// load single samples
template <bool REAL, bool CHAN, int FMT>
__device__ __forceinline__ void pfbg_body(const PfbgParams &pp)
{
#pragma clang fp contract(fast)
    const PfbmParams &p = pp.m;
    constexpr int NTH = kPfbgThreads, CH = CHAN ? kPfbgCols : 8, HALO = CHAN ? 1 : 0;
    const int M = p.M, D = p.D, Q = p.Q, nsel = p.nsel, ng = pp.ng;
    const int UP = 8 * ng + 4;                                   // floats per U row
    HIP_DYNAMIC_SHARED(float4, lds4)
    const int N4 = (D * (CH - 1) + Q * M + 3) / 2;               // 16-byte pieces of a chunk's input span
    float *xs = (float *)lds4;                                   // [2 N4] samples
    float *s_taps = xs + 4 * N4;                                 // [Q M] (REAL) or [Q M][2]
    float *U = s_taps + (((REAL ? 1 : 2) * Q * M + 3) & ~3);     // [32][UP]
    float *s_d = U, *s_m = U + kPfbgCols * kPfbgDS;              // [32][kPfbgDS] each (CHAN), once the pass's U is dead
    const int l = (int)threadIdx.x, lane = l & 63, n = lane & 31, kh = lane >> 5;
#if defined(__HIP_DEVICE_COMPILE__)
    const int wave = __builtin_amdgcn_readfirstlane(l >> 6);
#else
    const int wave = l >> 6;
#endif
    // ---- A: this wave's 32 rows of the DFT, all of K; the groups past ng are never used
    float4 a[kPfbgNG];
#pragma unroll
    for (int g = 0; g < kPfbgNG; g++) a[g] = pp.arows[((size_t)wave * ng + (g < ng ? g : ng - 1)) * 64 + lane];
    for (int i = l; i < Q * M; i += NTH) {
        if (REAL) s_taps[i] = ((const float *)p.taps)[2 * i];
        else { s_taps[2 * i] = ((const float *)p.taps)[2 * i]; s_taps[2 * i + 1] = ((const float *)p.taps)[2 * i + 1]; }
    }
    const long long tr0 = (long long)blockIdx.x * pp.run, tr1 = tr0 + pp.run;      // this workgroup's new instants
    const int npass = (pp.run + HALO + kPfbgCols - 1) / kPfbgCols;
    float prev[16];                                              // the previous pass's last column, in the accumulator's layout
#pragma unroll
    for (int i = 0; i < 16; i++) prev[i] = 0.f;
    // the tile sums' lane (l = channel): its place in the 50-instant grid and the sums so far
    int rr = 0, tile = (int)(tr0 / (p.TT > 0 ? p.TT : 1));
    double sacc = 0.0, hacc = 0.0;
    const DemodConst kc = demod_constants(p.gain);

    for (int ps = 0; ps < npass; ps++) {
        const long long tp0 = tr0 - HALO + (long long)ps * kPfbgCols;             // instant of column 0
        for (int ck = 0; ck < kPfbgCols / CH; ck++) {
            // ---- 0: the chunk's input span (16-byte aligned start)
            const long long gs = p.x0 + (long long)D * (tp0 + ck * CH);
            const long long a0 = gs & ~1LL;
            const int shift = (int)(gs - a0);
            const bool interior = a0 >= 0 && a0 + 2LL * N4 <= p.x_len;
            for (int i0 = 0; i0 < N4; i0 += 4 * NTH) {
                float4 v[4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int i = i0 + l + j * NTH < N4 ? i0 + l + j * NTH : N4 - 1;
                    if (interior) { if constexpr (FMT != kInF32) v[j] = load_sample_pair<FMT>(p.x, a0 + 2LL * i); else v[j] = ((const float4 *)(p.x + a0))[i]; }
                    else {
                        const long long s0 = a0 + 2LL * i, s1 = s0 + 1;
                        const bool in0 = s0 >= 0 && s0 < p.x_len, in1 = s1 >= 0 && s1 < p.x_len;
                        const float2 q0 = load_sample<FMT>(p.x, in0 ? s0 : 0), q1 = load_sample<FMT>(p.x, in1 ? s1 : 0);
                        v[j] = make_float4(in0 ? q0.x : 0.f, in0 ? q0.y : 0.f, in1 ? q1.x : 0.f, in1 ? q1.y : 0.f);
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; j++) { const int i = i0 + l + j * NTH; if (i < N4) ((float4 *)xs)[i] = v[j]; }
            }
            __syncthreads();
            // ---- A: branch filters, lane = (instant tl of the chunk, branch br)
            for (int i = l; i < CH * M; i += NTH) {
                const int tl = i / M, br = i - tl * M;
                const float *z = xs + 2 * (shift + D * tl + br);
                float ur = 0.f, ui = 0.f;
                for (int q = 0; q < Q; q++) {
                    const float2 v = *(const float2 *)(z + 2 * q * M);
                    if (REAL) { const float t = s_taps[q * M + br]; ur = t * v.x + ur; ui = t * v.y + ui; }
                    else {
                        const float2 t = *(const float2 *)(s_taps + 2 * (q * M + br));
                        ur = t.x * v.x + ur; ur = -t.y * v.y + ur;
                        ui = t.x * v.y + ui; ui = t.y * v.x + ui;
                    }
                }
                float *u = U + (ck * CH + tl) * UP;
                *(float2 *)(u + 2 * br) = make_float2(ur, ui);
                if (br == M - 1 && 8 * ng > 2 * M) *(float4 *)(u + 2 * M) = make_float4(0.f, 0.f, 0.f, 0.f);   // K's pad: A is zero there, B must be finite
            }
            __syncthreads();
        }
        // ---- B: the DFT of the pass's 32 instants
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; i++) acc[i] = 0.f;
        {
            const float *bp = U + n * UP + 4 * kh;
            float4 bn = *(const float4 *)bp;
#pragma unroll
            for (int g = 0; g < kPfbgNG; g++) {
                if (g < ng) {                                      // uniform
                    const float4 bv = bn;
                    bn = *(const float4 *)(bp + 8 * (g + 1 < ng ? g + 1 : g));
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g].x, bv.x, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g].y, bv.y, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g].z, bv.z, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g].w, bv.w, acc, 0, 0, 0);
                }
            }
        }
        // ---- C.  C/D layout: register 4 j + e = row 8 j + 4 kh + e of column n, i.e. for k = 2 j + h the lane holds channel
        // cl = 4 j + 2 kh + h of the wave's 16: re in register 4 j + 2 h, im in the next
        const long long t = tp0 + n;
        const bool live = t >= tr0 && t < tr1 && t < p.T;
        const int ph = (int)((t < 0 ? 0 : t) % (p.rot_period > 0 ? p.rot_period : 1));
        if (CHAN) __syncthreads();                                 // every wave has read its U: the angle / |Y|^2 tiles go on top
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int ir = 4 * (k >> 1) + 2 * (k & 1);
            const int c = 16 * wave + 4 * (k >> 1) + 2 * kh + (k & 1), cc = c < nsel ? c : nsel - 1;
            const float yr = acc[ir], yi = acc[ir + 1];
            if (CHAN) {
                float br = __shfl_up(yr, 1, 64), bi = __shfl_up(yi, 1, 64);       // Y[t - 1]: the left neighbour's
                if (n == 0) { br = prev[ir]; bi = prev[ir + 1]; }
                prev[ir] = __shfl(yr, (lane & 32) | 31, 64); prev[ir + 1] = __shfl(yi, (lane & 32) | 31, 64);
                const float2 rho = p.rho[cc];
                const float cr = br * rho.x + bi * rho.y, ci = bi * rho.x - br * rho.y;          // Y[t - 1] conj(rho)
                const float pr = yr * cr + yi * ci, pi = yi * cr - yr * ci;                      // Y[t] conj(Y[t - 1]) rho
                s_d[n * kPfbgDS + c] = demod_poly(kc, pr, pi);
                s_m[n * kPfbgDS + c] = live ? yr * yr + yi * yi : 0.f;
            }
            if (p.Z && live && c < nsel) {                         // the noise bank's output; channel bank: BTGPU_FLAG_DEBUG_Y
                const float2 kr = p.krot[(size_t)c * p.rot_period + ph];
                p.Z[(size_t)c * p.zstride + t] = make_float2(yr * kr.x - yi * kr.y, yr * kr.y + yi * kr.x);
            }
        }
        if (CHAN) {
            __syncthreads();
            // angles: rows of nsel floats -> d[t][drow]
            for (int i = l; i < kPfbgCols * nsel; i += NTH) {
                const int r = i / nsel, c = i - r * nsel;
                const long long t2 = tp0 + r;
                if (t2 >= tr0 && t2 < tr1 && t2 < p.T) p.d[(size_t)t2 * p.drow + c] = s_d[r * kPfbgDS + c];
            }
            // tile sums, lane = channel: the run's instants in order
            if (l < nsel) {
                const int hr = p.tail % p.TT;
                for (int r = 0; r < kPfbgCols; r++) {
                    const long long t2 = tp0 + r;
                    if (t2 < tr0 || t2 >= tr1) continue;
                    const float mm = s_m[r * kPfbgDS + l];
                    sacc += (double)mm;
                    if (hr > 0 && rr < hr && tile % p.tiles_per_block == p.tail / p.TT) hacc += (double)mm;
                    if (++rr == p.TT) {
                        if (tile < p.ntiles) { p.ptile[(size_t)l * p.ntiles + tile] = sacc; p.phead[(size_t)l * p.ntiles + tile] = hacc; }
                        rr = 0; tile++; sacc = 0.0; hacc = 0.0;
                    }
                }
            }
            // (the next pass writes U behind its staging barrier)
        }
    }
}

template <bool REAL, bool CHAN>
__global__ __launch_bounds__(kPfbgThreads) void pfbg_kernel(PfbgParams p)
{
    pfbg_body<REAL, CHAN, kInF32>(p);
}
template <bool REAL, bool CHAN>
__global__ __launch_bounds__(kPfbgThreads) void pfbg_kernel_s16(PfbgParams p)
{
    pfbg_body<REAL, CHAN, kInS16>(p);
}
template <bool REAL, bool CHAN>
__global__ __launch_bounds__(kPfbgThreads) void pfbg_kernel_s8(PfbgParams p)
{
    pfbg_body<REAL, CHAN, kInS8>(p);
}

// ---- launches.  L(kernel, grid, threads, lds_bytes, params) performs one; B is bank_launch.h's BankBuffers, arows the bank's
// pack_dft_rows on the device.  (Kept here: bank_launch.h is also compiled for the host emulator, which has no wave shuffles.)
template <class Launcher, class B>
inline int launch_channel_bank_g(const Design &des, const FastPath &fp, const B &b, const float4 *arows, size_t x_len,
                                 long long w0, long long G, Launcher &&L, int fmt = 0)
{
    const btgpu_design &d = des.d;
    const PfbBank &bk = fp.channel;
    PfbgParams g{};
    PfbmParams &p = g.m;
    p.x = b.x; p.x_len = (long long)x_len; p.x0 = w0 + d.first_channel_sample;
    p.M = bk.M; p.D = bk.D; p.Q = bk.Q; p.T = G; p.TT = pfbm_tile(bk.M);
    p.taps = b.taps_ch; p.nsel = d.high_channel - d.low_channel + 1;
    p.rho = b.rho_ch; p.rho_real = bk.rho_real ? 1 : 0;
    p.krot = b.krot_ch; p.rot_period = bk.rot_period;
    p.ntiles = (int)((G + p.TT - 1) / p.TT);
    p.d = b.d; p.drow = b.drow; p.ptile = b.ptile; p.phead = b.phead;
    p.tiles_per_block = des.outs_per_slot / p.TT; p.tail = des.tail;
    p.gain = des.demod_gain;
    p.Z = b.Ydebug; p.zstride = b.ystride;
    g.arows = arows; g.ng = pfbg_groups(bk.M);
    const int kt = pfbg_run_tiles(p.ntiles);
    g.run = kt * p.TT;
    const size_t lds = pfbg_lds_bytes(bk.M, bk.D, bk.Q, true, bk.real_taps);
    const int grid = (p.ntiles + kt - 1) / kt;
    if (bk.real_taps) L(BTGPU_KIN(fmt, pfbg_kernel, true, true), grid, kPfbgThreads, lds, g);
    else L(BTGPU_KIN(fmt, pfbg_kernel, false, true), grid, kPfbgThreads, lds, g);
    return p.ntiles;
}

template <class Launcher, class B>
inline void launch_noise_bank_g(const Design &des, const FastPath &fp, const B &b, const float4 *arows, size_t x_len,
                                long long w0, int S, Launcher &&L, int fmt = 0)
{
    const btgpu_design &d = des.d;
    const NoiseStage &ns = fp.noise;
    const PfbBank &bk = ns.pfb;
    PfbgParams g{};
    PfbmParams &p = g.m;
    p.x = b.x; p.x_len = (long long)x_len;
    p.x0 = w0 + d.first_noise_sample - ns.pad - (long long)ns.Jm * ns.R;
    p.M = bk.M; p.D = bk.D; p.Q = bk.Q; p.TT = pfbm_tile(bk.M);
    p.T = (long long)ns.outs * (S - 1) + ns.nw + ns.L3 - 1;
    p.taps = b.taps_n; p.nsel = d.high_channel - d.low_channel + 1;
    p.krot = b.krot_n; p.rot_period = bk.rot_period;
    p.ntiles = (int)((p.T + p.TT - 1) / p.TT);
    p.Z = b.Z; p.zstride = b.zstride;
    g.arows = arows; g.ng = pfbg_groups(bk.M);
    g.run = kPfbgNoiseRun;
    L(BTGPU_KIN(fmt, pfbg_kernel, false, false), (int)((p.T + g.run - 1) / g.run), kPfbgThreads,
      pfbg_lds_bytes(bk.M, bk.D, bk.Q, false, false), g);
}

}  // namespace btgpu
