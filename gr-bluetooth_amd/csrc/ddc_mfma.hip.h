// ddc_mfma.hip.h -- the direct-form decimating FIR bank (kernels.hip.h K1, ddc_direct_body) on the fp32 MATRIX pipe.
//
//     Y[c][g] = ( sum_j taps[c][j] * x[first + g D + j] ) * rot[c][g]
//
// for any decimation D >= 2, any whole number NB = ntp / D of tap blocks (14 for the channel bank, several hundred for the
// noise bank), 1 .. 79 channels, on the shared grid or with segmented addressing, both rotator forms, float32 or int16 input:
// the same arguments in meaning as ddc_direct_kernel and the same outputs BIT FOR BIT, so energy_kernel and demod_rows_kernel
// consume its Y unchanged.
//
// The shape is exact_dense.hip.h's:
//     M = (channel, re / im): 16 channels per 32-row block, exact_pack_taps_dense's signs and swaps
//     N = output instants: wave w owns the tile's columns [32 w, 32 w + 32), 128 consecutive outputs of ONE segment per workgroup
//     K = the 2 D floats of ONE tap block q; the accumulator starts at +0 for every q, the block's result is added to y on the
//         vector ALU, q ascending (y = G[0], then y = y + G[q]): the oracle's summation order (exact.hip.h)
// Only v_mfma_f32_32x32x2_f32 is used (the instruction whose chain was checked on the device), under fp contract(off).
//
// What is its own:
//
// (1) A RING of staged input in LDS, marched along the taps.  Output u of the tile and tap block q read column u + q of the input
// reshaped into columns of D samples; 128 + NB - 1 columns are several hundred KB at the noise bank's NB.  The taps are taken in
// CHUNKS of QC <= 16 blocks; a chunk needs the 127 + QC columns [q0, q0 + QC + 127), which is the ring: column m lives in slot
// m % (127 + QC), in exact_dense's conflict-free layout [column][re | im][r] with the column stride 2 dpad + 4 floats.  Going to
// the next chunk retires QC columns and brings QC new ones into the very slots retired: their samples are loaded into registers
// (raw, i.e. 4 bytes per int16 sample, 2 per int8 sample; kDmPF per lane, all in flight at once) when the current chunk BEGINS and are written to LDS
// between two barriers when it ends -- QC NI nblk 4 matrix instructions later.  61.8 KB at D = 50: two workgroups per CU.
// Outside the input (a < 0, a >= x_len) the samples are zeros, the loads clamped, as in the VALU form.
// (Single samples, not InPiece pairs: a column's first sample has either parity (odd D, odd `first`), and the float stream's
// base is only 8-byte aligned in btgpu_process_device; the staging is 1 / 1000 of the kernel's instructions either way.)
//
// (2) SEVERAL row blocks of a column set in registers: y and the running block sum G of kDmRB = 3 row blocks are 2 x 3 x 16
// accumulator registers; one 16-byte B read from LDS feeds every row block's four matrix instructions.  grid.y takes the row
// blocks in groups of three: 79 channels (five row blocks) are 3 + 2, the input is staged from HBM twice per tile, not five
// times.  Not all five: y and G for five row blocks, two sets of taps and the raw samples compiled to 256 VGPRs with 336 bytes
// of scratch memory under the two-workgroups-per-CU bound, four row blocks to 120 bytes; three take 214 VGPRs (210 for int16) and none.
//
// (3) The tap stream.  The A operand is ONE linear stream per workgroup in the order of use, [tap block q][group i][row block b]
// [lane][4 steps] (pack_direct_mfma_taps, design_fast.cc), read by all four waves: 1 KB per row block and group from the L1 / L2.
// It is kept TWO groups ahead in two register sets that take turns by a loop unrolled twice (no rotating copy: a copy under a
// run-time trip count compiles to moves behind vmcnt(0), exact_dense.hip.h), each set re-loaded right behind the matrix
// instructions that consumed it: up to 2 x 4 x 3 matrix instructions (1536 cycles) cover a load.  The loads are
// unconditional (row blocks past the handle's last re-read its last word), so that the wait counts stay static.
// A word feeds ONE column set per wave here, not two: beside y and G of three row blocks a second column set (another 96
// accumulator registers) does not fit two workgroups per CU, and the four waves of a workgroup -- and the
// workgroups of a CU, which march through the taps in step -- read the same words, so HBM / L2 see a word once per tile and
// chunk; DESIGN.md section 4.1 has the measured rates of the channel bank (taps stay in the L2) against the noise bank (tens of MB).
//
// Epilogue: in the C/D layout a lane holds re and im of eight channels of its column; de-rotation is ddc_direct_body's,
// verbatim, and the float2 stores are 256-byte runs per half-wave along g.  Outputs past seg_len / G and channels past nch
// are masked.
#pragma once
#include <algorithm>

#include "exact.hip.h"

namespace btgpu {

constexpr int kDmThreads = 256, kDmCols = 128;  // four waves of 32 columns
constexpr int kDmRB = 3;                        // row blocks (of 16 channels) held in registers per workgroup
constexpr int kDmQCMax = 16;                    // tap blocks per chunk of the ring, at most
constexpr int kDmPF = 4;                        // raw samples per lane in flight for the next chunk: QC D <= kDmPF kDmThreads
constexpr int kDmAhead = 2;                     // groups the A stream is read ahead (zero words behind the packed taps)
constexpr size_t kDmLdsBudget = 80 * 1024;      // two workgroups per CU

struct DdcMfmaParams {
    const float2 *x; long long x_len;
    long long first;              // x index of (output 0, tap 0)
    int D, NB, QC;                // decimation, tap blocks ntp / D, tap blocks per chunk (ddc_mfma_chunk)
    const float *taps;            // pack_direct_mfma_taps
    const float2 *rot; int Q;     // de-rotation table [nch][Q], or Q == 0:
    const double *rot_step_turns; // ... the phase step per output in turns, [nch]
    float2 *Y; long long G, ystride;
    int nch;
    int seg_len; long long seg_stride;   // seg_len > 0: segmented outputs (one segment per window), as in ddc_direct_body
};

inline size_t ddc_mfma_lds_bytes(int D, int QC) { return (size_t)(kDmCols - 1 + QC) * (2 * exact_dpad(D) + 4) * sizeof(float); }
// tap blocks per chunk: as many as the lanes' kDmPF raw samples and the LDS budget hold; 0 = this decimation is not served
inline int ddc_mfma_chunk(int D, int NB)
{
    if (D < 2 || NB < 1) return 0;
    int qc = std::min(std::min(kDmQCMax, NB), kDmPF * kDmThreads / D);
    while (qc > 0 && ddc_mfma_lds_bytes(D, qc) > kDmLdsBudget) qc--;
    return qc;
}

template <int FMT> struct DmRaw { typedef float2 type; };
template <> struct DmRaw<kInS16> { typedef uint32_t type; };
template <> struct DmRaw<kInS8> { typedef uint16_t type; };      // one int8 sample: a 16-bit load, one register where the float form takes two
template <int FMT>
__device__ __forceinline__ typename DmRaw<FMT>::type dm_load_raw(const float2 *x, long long i)
{
    if constexpr (FMT == kInS16) return ((const uint32_t *)x)[i];
    else if constexpr (FMT == kInS8) return ((const uint16_t *)x)[i];
    else return x[i];
}
__device__ __forceinline__ float2 dm_widen(const float2 &v) { return v; }
__device__ __forceinline__ float2 dm_widen(uint32_t w) { return s16_widen(w); }
__device__ __forceinline__ float2 dm_widen(uint16_t h) { return s8_widen(h); }

template <int FMT>
__device__ __forceinline__ void ddc_mfma_body(const DdcMfmaParams &p)
{
#pragma clang fp contract(off)
    HIP_DYNAMIC_SHARED(float2, lds)
    float *Bs = (float *)lds;                                      // [127 + QC][CS]
    const int D = p.D, DP = exact_dpad(D), NI = DP >> 2, CS = 2 * DP + 4;
    const int rem = D - 4 * (NI - 1);                              // matrix instructions of a tap block's last group: none for a pad step
    const int NB = p.NB, QC = p.QC, R = kDmCols - 1 + QC;
    const int tid = (int)threadIdx.x, lane = tid & 63;
#if defined(__HIP_DEVICE_COMPILE__)
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#else
    const int wave = tid >> 6;
#endif
    const int n = lane & 31, kh = lane >> 5;
    const int u = 32 * wave + n;                                   // this lane's column = output u of the tile
    const int tiles_per_seg = p.seg_len > 0 ? (p.seg_len + kDmCols - 1) / kDmCols : 0;
    const long long seg = p.seg_len > 0 ? (long long)(blockIdx.x / tiles_per_seg) : 0;
    const long long g0 = p.seg_len > 0 ? (long long)(blockIdx.x % tiles_per_seg) * kDmCols : (long long)blockIdx.x * kDmCols;
    const long long base = p.first + seg * p.seg_stride + g0 * D;  // sample (column 0, step 0) of the tile
    const int b0 = (int)blockIdx.y * kDmRB;
    const int nbh = min(kDmRB, exact_dense_blocks(p.nch) - b0);    // row blocks of this workgroup

    // ---- the first chunk's columns [0, nq + 127): sample s = (column s / D, step s % D), consecutive lanes consecutive samples ----
    {
        const int total = (min(QC, NB) + kDmCols - 1) * D, dm = kDmThreads / D, dr = kDmThreads - dm * D;
        int m = tid / D, r = tid - m * D;
        const bool inside = base >= 0 && base + total <= p.x_len;  // uniform
        for (int s = tid; s < total; s += kDmThreads) {
            float2 v;
            if (inside) v = load_sample<FMT>(p.x, base + s);
            else {
                const long long a = base + s;
                v = load_sample<FMT>(p.x, a < 0 ? 0 : (a < p.x_len ? a : p.x_len - 1));
                if (!(a >= 0 && a < p.x_len)) v = make_float2(0.f, 0.f);
            }
            Bs[m * CS + r] = v.x;
            Bs[m * CS + DP + r] = v.y;
            m += dm; r += dr;
            if (r >= D) { r -= D; m++; }
        }
    }
    // ---- the ring: the chunk that starts at tap block q1 brings the columns [q1 + 127, q1 + 127 + nq1) ----
    typename DmRaw<FMT>::type raw[kDmPF];
    auto prefetch = [&](int q1) {
        const long long a0 = base + (long long)(q1 + kDmCols - 1) * D + tid;
#pragma unroll
        for (int k = 0; k < kDmPF; k++) {                          // unconditional, clamped: all in flight together
            const long long a = a0 + k * kDmThreads;
            raw[k] = dm_load_raw<FMT>(p.x, a < 0 ? 0 : (a < p.x_len ? a : p.x_len - 1));
        }
    };
    auto commit = [&](int q1) {
        const int total = min(QC, NB - q1) * D;
        const long long a0 = base + (long long)(q1 + kDmCols - 1) * D;
#pragma unroll
        for (int k = 0; k < kDmPF; k++) {
            const int s = tid + k * kDmThreads;
            if (s < total) {
                const int mm = (int)((unsigned int)s / (unsigned int)D), r = s - mm * D;
                const int sl = (int)((unsigned int)(q1 + kDmCols - 1 + mm) % (unsigned int)R);
                const long long a = a0 + s;
                const float2 v = (a >= 0 && a < p.x_len) ? dm_widen(raw[k]) : make_float2(0.f, 0.f);
                Bs[sl * CS + r] = v.x;
                Bs[sl * CS + DP + r] = v.y;
            }
        }
    };
    if (QC < NB) prefetch(QC);

    // ---- A: the linear tap stream, two groups ahead in two register sets ----
    const int aw = nbh * 64;                                       // 16-byte words of one group (q, i)
    const float4 *apA = (const float4 *)p.taps + (size_t)b0 * NB * NI * 64 + lane, *apB = apA + aw;
    float4 aA[kDmRB], aB[kDmRB];
#pragma unroll
    for (int j = 0; j < kDmRB; j++) { aA[j] = apA[(j < nbh ? j : nbh - 1) * 64]; aB[j] = apB[(j < nbh ? j : nbh - 1) * 64]; }
    apA += 2 * aw; apB += 2 * aw;

    f32x16 y[kDmRB], acc[kDmRB];
#pragma unroll
    for (int j = 0; j < kDmRB; j++)
#pragma unroll
        for (int e = 0; e < 16; e++) { y[j][e] = 0.f; acc[j][e] = 0.f; }
    int q = 0, qc = 0, i = 0;                                      // tap block, its index in the chunk, group of the block (uniform)
    int sl = u;                                                    // slot of this lane's column u + q
    __syncthreads();
    const float *bp = Bs + kh * DP;
    float4 bn = *(const float4 *)(bp + sl * CS);

    auto step = [&](float4 (&a)[kDmRB], const float4 *&ap) {
        if (i == 0) {
            if (qc == QC) {                                        // the chunk is done: march the ring
                qc = 0;
                __syncthreads();                                   // (every wave has read the retired columns)
                commit(q);
                __syncthreads();
                if (q + QC < NB) prefetch(q + QC);
                bn = *(const float4 *)(bp + sl * CS);              // (column 127 + q is a new one)
            }
#pragma unroll
            for (int j = 0; j < kDmRB; j++)
#pragma unroll
                for (int e = 0; e < 16; e++) acc[j][e] = 0.f;
        }
        const float4 bv = bn;
        const bool last = i == NI - 1;
        const int sl1 = sl + 1 == R ? 0 : sl + 1;
        bn = *(const float4 *)(bp + (last ? sl1 * CS : sl * CS + 4 * (i + 1)));    // the next group's B (behind the last tap block: read, unused)
        if (!last) {                                               // (two code paths, not a branch per matrix instruction)
#pragma unroll
            for (int j = 0; j < kDmRB; j++)
                if (j < nbh) {                                     // uniform
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].x, bv.x, acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].y, bv.y, acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].z, bv.z, acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].w, bv.w, acc[j], 0, 0, 0);
                }
        } else {
#pragma unroll
            for (int j = 0; j < kDmRB; j++)
                if (j < nbh) {
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].x, bv.x, acc[j], 0, 0, 0);
                    if (rem > 1) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].y, bv.y, acc[j], 0, 0, 0);
                    if (rem > 2) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].z, bv.z, acc[j], 0, 0, 0);
                    if (rem > 3) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].w, bv.w, acc[j], 0, 0, 0);
                }
        }
#pragma unroll
        for (int j = 0; j < kDmRB; j++) a[j] = ap[(j < nbh ? j : nbh - 1) * 64];   // this set's next group, two ahead
        ap += 2 * aw;
        __builtin_amdgcn_sched_barrier(0);                         // (keep the loads HERE, ahead of their use: exact.hip.h)
        if (last) {
            if (q == 0) {
#pragma unroll
                for (int j = 0; j < kDmRB; j++) y[j] = acc[j];
            } else {
#pragma unroll
                for (int j = 0; j < kDmRB; j++)
#pragma unroll
                    for (int e = 0; e < 16; e++) y[j][e] = y[j][e] + acc[j][e];
            }
            i = 0; q++; qc++; sl = sl1;
        } else i++;
    };
    const int T = NB * NI;
    for (int t = 0; t < T; t += 2) {
        step(aA, apA);
        if (t + 1 < T) step(aB, apB);
    }

    // ---- epilogue.  C/D layout: register 4 j4 + e = row 8 j4 + 4 kh + e of column n, i.e. for k = 2 j4 + h the lane holds
    // channel cl = 4 j4 + 2 kh + h of the row block: re in register 4 j4 + 2 h, im in the next ----
    const long long g = g0 + u;                                    // index inside the segment (or on the shared grid)
    if (p.seg_len > 0 ? g >= p.seg_len : g >= p.G) return;
    const long long gout = p.seg_len > 0 ? seg * p.seg_len + g : g;
#pragma unroll
    for (int j = 0; j < kDmRB; j++) {
        if (j >= nbh) break;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int c = kExDenseRows * (b0 + j) + 4 * (k >> 1) + 2 * kh + (k & 1);
            if (c >= p.nch) continue;
            const float yr = y[j][4 * (k >> 1) + 2 * (k & 1)], yi = y[j][4 * (k >> 1) + 2 * (k & 1) + 1];
            float rr, ri;
            if (p.Q > 0) {
                const float2 rt = p.rot[(size_t)c * p.Q + (int)(g % p.Q)];
                rr = rt.x; ri = rt.y;
            } else {
                double t = p.rot_step_turns[c] * (double)g;
                t -= floor(t);
                double s, co;
                sincospi(2.0 * t, &s, &co);
                rr = (float)co; ri = (float)s;
            }
            float2 out;
            out.x = fmaf(-yi, ri, yr * rr);
            out.y = fmaf(yi, rr, yr * ri);
            p.Y[(size_t)c * p.ystride + gout] = out;
        }
    }
}

__global__ __launch_bounds__(kDmThreads, 2) void ddc_mfma_kernel(DdcMfmaParams p) { ddc_mfma_body<kInF32>(p); }
// (a template only so that it can be instantiated in the int16 kernels' translation unit: s16_inst.h)
template <int V = 0>
__global__ __launch_bounds__(kDmThreads, 2) void ddc_mfma_kernel_s16(DdcMfmaParams p) { ddc_mfma_body<kInS16>(p); }
template <int V = 0>
__global__ __launch_bounds__(kDmThreads, 2) void ddc_mfma_kernel_s8(DdcMfmaParams p) { ddc_mfma_body<kInS8>(p); }

}  // namespace btgpu
