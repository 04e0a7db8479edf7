// payload_sweep.hip.h -- the payload CRC of every classic hit under the 64 CLK1-6 candidates (second half).
//
// What basic_rate_piconet::UAP_from_header asks of a packet beside try_clock(clock) (header_sweep_kernel) is
// classic_packet::crc_check(clock) (lib/packet_impl.cc:612-671 with :675-1043 behind it): FEC 2/3 decoding, unwhitening with the
// candidate clock's sequence, the payload header's length, a CRC-16 -- 64 times per packet.  Most of that does not depend on the
// clock, so one wave per hit does it ONCE (phase A, lanes cooperate) and only then splits into lane = clock (phase B):
//
//   phase A   the record's payload symbols re-aligned to bit 0 and masked to `length`, as packed words in LDS (stream PAY);
//             the (15,10) code with lane = codeword, up to three passes of the wave for the 183 codewords of a DM5: 15 bits
//             out of two words, the five parity bits as parities of masked words, the mismatch count a popcount; the ten data
//             bits of each codeword OR-ed into a second packed stream (DEC); the first failing codeword by ballot + ctz.  The
//             same for the ten DV-aligned codewords (80 voice symbols later: stream DVD) where some lane's type is 8, and the
//             HV1 majority vote where some lane's type is 5.
//   phase B   lane = clock: the whitening sequence (period 127) as a 127-entry table of 32-bit windows in LDS, the lane's
//             window index advanced by 32 mod 127 per word; the payload header gives the lane's own length, bound-checked as
//             the reference does; then the CRC-16 a byte at a time through a 256-entry table in LDS, over the wave's longest
//             length with each lane comparing at its own byte.  Every lane of one packet type reads the same data word in the
//             same iteration (an LDS broadcast); the per-lane addresses are the whitening window and the CRC table.
//             FHS: crc(d ^ w, init) = crc(d ^ w, 0) ^ advance(init), so the 64 residues R[c] = crc(d ^ w_c, 0) ^ check_c are
//             formed once and each lane compares its own advance(init(UAP)) with R[own] and R[32..63] (the reference's retry).
//
// This is the straightforward per-lane CRC of the two forms the design allows: the data part of the CRC is NOT split off.
// Quirks of the reference restated here are listed at the places they act; the oracle is oracle/bt_uap.c.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "kernels.hip.h"

namespace btgpu {

struct PayloadRec { int16_t verdict[64]; int32_t length; int32_t pad_; };   // == btgpu_crc_sweep
static_assert(sizeof(PayloadRec) == 136 && sizeof(PayloadRec) % 8 == 0, "136 bytes, whole 8-byte pieces");

constexpr int kPsWords = 92;          // words per packed stream: 2745 symbols = 86 words, + the look-ahead of extraction
constexpr int kPsMaxCw = 183;         // codewords of the longest FEC 2/3 payload (DM5: 228 bytes)

// ---- compile-time tables: the whitening sequence, the start of each clock's sequence in it, the byte-wise CRC-16 ----
struct PsTables {
    uint32_t win[127];                // win[k] bit j = sequence bit (k + j) mod 127
    uint8_t  start[64];               // where the sequence of CLK1-6 = c begins (classic_packet::INDICES)
    uint16_t crc[256];                // reflected CRC-16, polynomial 0x8408 (crcgen, lib/packet_impl.cc:529-548, eight bits at once)
};

constexpr PsTables ps_make_tables()
{
    PsTables t{};
    // x^7 + x^4 + 1 from register (0,0,0,0,0,0,1): w[i] = w[i-7] ^ w[i-3] (lib/packet_impl.cc:84-90 regenerated from its rule)
    uint8_t w[127] = {};
    uint8_t p[7] = {0, 0, 0, 0, 0, 0, 1};
    for (int i = 0; i < 127; i++) {
        const uint8_t o = p[6];
        w[i] = o;
        const uint8_t q[7] = {o, p[0], p[1], p[2], (uint8_t)(p[3] ^ o), p[4], p[5]};
        for (int k = 0; k < 7; k++) p[k] = q[k];
    }
    for (int k = 0; k < 127; k++) {
        uint32_t v = 0;
        for (int j = 0; j < 32; j++) v |= (uint32_t)w[(k + j) % 127] << j;
        t.win[k] = v;
    }
    for (int c = 0; c < 64; c++) {
        uint8_t r[7] = {(uint8_t)(c & 1), (uint8_t)((c >> 1) & 1), (uint8_t)((c >> 2) & 1), (uint8_t)((c >> 3) & 1),
                        (uint8_t)((c >> 4) & 1), (uint8_t)((c >> 5) & 1), 1};
        uint32_t s = 0;
        for (int k = 0; k < 7; k++) {
            const uint8_t o = r[6];
            s |= (uint32_t)o << k;
            const uint8_t q[7] = {o, r[0], r[1], r[2], (uint8_t)(r[3] ^ o), r[4], r[5]};
            for (int m = 0; m < 7; m++) r[m] = q[m];
        }
        for (int i = 0; i < 127; i++) if ((t.win[i] & 0x7fu) == s) { t.start[c] = (uint8_t)i; break; }
    }
    for (int x = 0; x < 256; x++) {
        uint32_t r = (uint32_t)x;
        for (int k = 0; k < 8; k++) r = (r >> 1) ^ ((r & 1u) ? 0x8408u : 0u);
        t.crc[x] = (uint16_t)r;
    }
    return t;
}
__device__ const PsTables kPsTables = ps_make_tables();

// parity of the ten data bits: the register of lfsr(data, 15, 10, {1,1,0,1,0,1}) (lib/packet_impl.cc:278-307, :386-468)
constexpr uint32_t ps_fec23_parity(uint32_t data)
{
    uint32_t reg = 0;                                   // bit k = reg[k]
    for (int i = 9; i >= 0; i--) {
        const uint32_t fb = ((data >> i) ^ (reg >> 4)) & 1u;
        // reg[j] = reg[j-1] ^ (g[j] ? fb : 0) for j = 4..1 with g = 1,1,0,1,0; reg[0] = fb
        reg = ((reg << 1) & 0x1eu) ^ (fb ? 0x0bu : 0u);
    }
    return reg;
}
// ... which is linear: parity bit k = parity(data & ps_fec23_mask(k))
constexpr uint32_t ps_fec23_mask(int k)
{
    uint32_t m = 0;
    for (int i = 0; i < 10; i++) m |= ((ps_fec23_parity(1u << i) >> k) & 1u) << i;
    return m;
}

// `n` (<= 32) bits of a packed stream from bit `q` on; the stream has a readable word behind the last one used
__device__ __forceinline__ uint32_t ps_bits(const uint32_t *s, int q, int n)
{
    const int w = q >> 5, sh = q & 31;
    const uint64_t v = ((uint64_t)s[w + 1] << 32) | s[w];
    return (uint32_t)(v >> sh) & (n >= 32 ? 0xffffffffu : ((1u << n) - 1u));
}

// one codeword of the (15,10) code: its ten data bits, and whether two or more of its five parity bits disagree (the reference's
// "correction" can never match -- quirk Q12 of oracle/bt_uap.c -- so such a codeword fails and nothing is ever corrected)
__device__ __forceinline__ bool ps_codeword(const uint32_t *pay, int q, uint32_t &data)
{
    constexpr uint32_t m0 = ps_fec23_mask(0), m1 = ps_fec23_mask(1), m2 = ps_fec23_mask(2), m3 = ps_fec23_mask(3), m4 = ps_fec23_mask(4);
    const uint32_t cw = ps_bits(pay, q, 15);
    data = cw & 0x3ffu;
    const uint32_t par = (__popc(data & m0) & 1) | ((__popc(data & m1) & 1) << 1) | ((__popc(data & m2) & 1) << 2) |
                         ((__popc(data & m3) & 1) << 3) | ((__popc(data & m4) & 1) << 4);
    return __popc(par ^ (cw >> 10)) >= 2;
}

__device__ __forceinline__ int ps_wave_max(int v)
{
    for (int d = 32; d >= 1; d >>= 1) { const int o = __shfl_xor(v, d, 64); v = o > v ? o : v; }
    return v;
}

// One wave per hit, grid-strided over the hit list like header_sweep_kernel, behind it on the same stream: `hdr` is its output.
__global__ __launch_bounds__(64) void payload_sweep_kernel(
    const DeviceHit *__restrict__ hits, const unsigned int *__restrict__ hit_count, int max_hits,
    const uint32_t *__restrict__ symbits, const HeaderRec *__restrict__ hdr, int to_header,
    PayloadRec *__restrict__ out)
{
    __shared__ uint32_t strm[3 * kPsWords];             // PAY | DEC | DVD
    __shared__ uint32_t win[127];
    __shared__ uint16_t crctab[256];
    __shared__ uint16_t fhs_r[64];
    uint32_t *const pay = strm, *const dec = strm + kPsWords, *const dvd = strm + 2 * kPsWords;
    const int lane = threadIdx.x;
    for (int k = lane; k < 127; k += 64) win[k] = kPsTables.win[k];
    for (int k = lane; k < 256; k += 64) crctab[k] = kPsTables.crc[k];
    int idx0 = kPsTables.start[lane] + 18;              // the payload follows the 18 header bits
    idx0 = idx0 >= 127 ? idx0 - 127 : idx0;
    unsigned int n = *hit_count;
    if (n > (unsigned int)max_hits) n = (unsigned int)max_hits;
    for (unsigned int i = blockIdx.x; i < n; i += gridDim.x) {
        const DeviceHit h = hits[i];
        PayloadRec *o = &out[i];
        int length = 0;
        if (h.sym >= 0) {
            length = h.nsym < 32 * kSymWords - h.offset ? h.nsym : 32 * kSymWords - h.offset;
            length = length < 0 ? 0 : length;
        }
        if (lane == 0) { o->length = length; o->pad_ = 0; }
        if (h.kind != 0 || h.sym < 0 || hdr[i].fec13_ok == 0) { o->verdict[lane] = -1; continue; }
        const int type = hdr[i].type[lane];
        const uint32_t uap = hdr[i].uap[lane];
        const int size = length - (to_header + 54);      // payload symbols the packet holds (may be negative)
        const uint32_t *row = symbits + (size_t)h.sym * kSymWords;
        __syncthreads();                                 // (the previous hit's phase B has left the streams)

        // ---------------- phase A: clock-independent ----------------
        {
            const int p0 = h.offset + to_header + 54, w0 = p0 >> 5, sh = p0 & 31;
            for (int k = lane; k < 3 * kPsWords; k += 64) {
                uint32_t v = 0;
                if (k < kPsWords && 32 * k < size) {
                    const uint32_t lo = w0 + k < kSymWords ? row[w0 + k] : 0u, hi = w0 + k + 1 < kSymWords ? row[w0 + k + 1] : 0u;
                    v = sh ? (lo >> sh) | (hi << (32 - sh)) : lo;
                    if (size - 32 * k < 32) v &= (1u << (size - 32 * k)) - 1u;   // symbols at positions >= length read as 0
                }
                strm[k] = v;
            }
        }
        __syncthreads();
        // codewords that hold a symbol at all (the others are zero: they decode to zeros and cannot fail)
        int ncw = size > 0 ? (size + 14) / 15 : 0;
        ncw = ncw > kPsMaxCw ? kPsMaxCw : ncw;
        int first_fail = 0x7fffffff;
        for (int b0 = 0; b0 < ncw; b0 += 64) {
            const int b = b0 + lane;
            uint32_t data = 0;
            const bool bad = b < ncw && ps_codeword(pay, 15 * b, data);
            if (b < ncw && data) {
                const int q = 10 * b, sh = q & 31;
                atomicOr(&dec[q >> 5], data << sh);
                if (sh > 22) atomicOr(&dec[(q >> 5) + 1], data >> (32 - sh));
            }
            const unsigned long long f = __ballot(bad);
            if (f && first_fail == 0x7fffffff) first_fail = b0 + __builtin_ctzll(f);
        }
        int first_fail_dv = 0x7fffffff;
        if (__ballot(type == 8)) {                       // DV: the data field follows 80 voice symbols
            uint32_t data = 0;
            const bool bad = lane < 10 && ps_codeword(pay, 80 + 15 * lane, data);
            if (lane < 10 && data) {
                const int q = 10 * lane, sh = q & 31;
                atomicOr(&dvd[q >> 5], data << sh);
                if (sh > 22) atomicOr(&dvd[(q >> 5) + 1], data >> (32 - sh));
            }
            const unsigned long long f = __ballot(bad);
            if (f) first_fail_dv = __builtin_ctzll(f);
        }
        bool hv1_ok = true;
        if (__ballot(type == 5) && size >= 240) {        // HV1: unfec13 over 240 symbols, ok iff fewer than 80 / 4 triples disagree
            int be = 0;
            for (int t0 = 0; t0 < 80; t0 += 64) {
                const int t = t0 + lane;
                const uint32_t v = t < 80 ? ps_bits(pay, 3 * t, 3) : 0u;
                be += __popcll(__ballot(v != 0u && v != 7u));
            }
            hv1_ok = be < 80 / 4;
        }
        __syncthreads();

        // ---------------- phase B: lane = clock ----------------
        // r: the verdict before the last two rules of crc_check; a CRC job compares at bytes mlo .. mhi of stream `src`
        int r = 1, mlo = 1, mhi = 0, src = 0;
        bool ev4_first = false, fhs_wait = false;
        const bool is_dm = type == 3 || type == 8 || type == 10 || type == 14;
        const bool is_dh = type == 4 || type == 9 || type == 11 || type == 15;
        if (type == 2) {                                                         // fhs(): :688-722
            if (size >= 240) { if (first_fail < 16) r = 0; else fhs_wait = true; }
        } else if (is_dm || is_dh) {                                             // DM(): :770-830, DH(): :834-884
            const int sz = type == 8 ? size - 80 : size;
            const int ff = type == 8 ? first_fail_dv : first_fail;
            const bool one = type == 3 || type == 8 || type == 4 || type == 9;   // one-byte payload header
            src = is_dh ? 0 : (type == 8 ? 2 * kPsWords : kPsWords);
            // decode_payload_header (:725-767): too short, or (FEC) its codewords fail -> 0
            const bool hdr_ok = is_dh ? sz >= (one ? 8 : 16) : (sz >= (one ? 15 : 30) && ff >= (one ? 1 : 2));
            if (!hdr_ok) r = 0;
            else {
                const uint32_t ph = strm[src] ^ win[idx0];
                const int pl = one ? (int)((ph >> 3) & 0x1fu) + 3 : (int)((ph >> 3) & 0x3ffu) + 4;
                const int mx = type == 8 ? 12 : type == 3 ? 20 : type == 10 ? 125 : type == 14 ? 228 : type == 11 ? 187 : type == 15 ? 343 : 30;
                if (pl > mx || 8 * pl > sz || type == 9) r = 1;                  // (AUX1 has no CRC)
                else if (is_dm && ff < (8 * pl + 9) / 10) r = 0;                 // unfec23 over ceil(bits / 10) codewords
                else { mlo = mhi = pl - 2; }
            }
        } else if (type == 12) {                                                 // EV4(): :917-969
            // block k (symbols 15k .., k <= 97) is reached iff it and all before it are whole and decode; with it the lengths
            // pl with 8 pl <= 10 k are tested.  Every other way out of the loop ends as 1.
            int kok = size / 15 - 1;
            kok = kok > 97 ? 97 : kok;
            kok = kok > first_fail - 1 ? first_fail - 1 : kok;
            if (size >= 15 && kok >= 1) {
                const int plmax = (10 * kok) / 8;                                // <= 121
                src = kPsWords; mlo = 0; mhi = plmax - 2;
                ev4_first = true;                                                // pl = 1: check bits in front of the payload read as 0
            }
        } else if (type == 5) {                                                  // HV(): :1003-1043
            if (size >= 240 && !hv1_ok) r = 0;
        }
        // (EV3 and EV5 end as 1 whatever they find; AUX1, HV2, HV3/EV3, NULL and POLL are not looked at)

        const uint32_t init = (__brev(uap) >> 24) << 8;
        bool ok = false;
        {
            uint32_t reg = init;
            int idx = idx0;
            uint32_t wa = win[idx], da = strm[src];
            if (ev4_first) ok = ((da ^ wa) & 0xffu) == (init >> 8);
            const int nw = ps_wave_max(mhi >= mlo ? (mhi >> 2) + 1 : 0);
            for (int j = 0; j < nw; j++) {
                idx = idx + 32 >= 127 ? idx + 32 - 127 : idx + 32;
                const uint32_t wb = win[idx], db = strm[src + j + 1];
                const uint64_t u = ((uint64_t)(db ^ wb) << 32) | (da ^ wa);
                for (int b = 0; b < 4; b++) {
                    const int m = 4 * j + b;
                    const uint32_t v = (uint32_t)(u >> (8 * b));
                    ok = ok || (m >= mlo && m <= mhi && reg == (v & 0xffffu));
                    reg = (reg >> 8) ^ crctab[(reg ^ v) & 0xffu];
                }
                wa = wb; da = db;
            }
        }
        if (mhi >= mlo || ev4_first) r = ok ? 10 : 1;

        if (__ballot(fhs_wait)) {
            // R[c] = crc(dec ^ w_c, 0) over 144 bits ^ the 16 bits behind them; lane c then wants R == advance(init) from its own
            // clock or from one of 32 .. 63 (fhs() tries those after the packet's own)
            uint32_t reg = 0, adv = init;
            int idx = idx0;
            uint32_t wa = win[idx], da = dec[0];
            for (int j = 0; j < 5; j++) {
                idx = idx + 32 >= 127 ? idx + 32 - 127 : idx + 32;
                const uint32_t wb = win[idx], db = dec[j + 1];
                const uint64_t u = ((uint64_t)(db ^ wb) << 32) | (da ^ wa);
                for (int b = 0; b < 4; b++) {
                    const uint32_t v = (uint32_t)(u >> (8 * b));
                    if (4 * j + b == 18) reg ^= v & 0xffffu;
                    if (4 * j + b < 18) { reg = (reg >> 8) ^ crctab[(reg ^ v) & 0xffu]; adv = (adv >> 8) ^ crctab[adv & 0xffu]; }
                }
                wa = wb; da = db;
            }
            fhs_r[lane] = (uint16_t)reg;
            __syncthreads();
            bool hit = reg == adv;
            for (int c = 32; c < 64; c++) hit = hit || fhs_r[c] == adv;
            if (fhs_wait) r = hit ? 1000 : 0;
        }
        // crc_check's last rules (:660-671): a refutation counts only for FHS, DM1 and HV1
        if (r == 0 && type != 2 && type != 3 && type != 5) r = 1;
        o->verdict[lane] = (int16_t)r;
    }
}

// The sweeps leave for the host as the header sweeps do (records_out_kernel, whose argument list the emulator compiles and which
// therefore stays as it is): the first min(count, cap) records straight into page-locked memory, 8 bytes per lane.
__global__ __launch_bounds__(256) void payload_out_kernel(const unsigned int *__restrict__ counts, int max_hits,
                                                          const uint2 *__restrict__ crc, uint2 *__restrict__ h_crc, unsigned int cap)
{
    unsigned int n = counts[0];
    n = n > (unsigned int)max_hits ? (unsigned int)max_hits : n;
    const size_t m = (size_t)(n < cap ? n : cap) * (sizeof(PayloadRec) / 8);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (size_t)gridDim.x * blockDim.x) h_crc[i] = crc[i];
}

}  // namespace btgpu
