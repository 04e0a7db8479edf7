// le_sweep.hip.h -- what lies behind every access-address hit: the dewhitened PDU header, its CRC-24, and the CRCInit it implies.
//
// le_packet::sniff_aa accepts on the preamble, the access address and the shape of the header; the reference never looks at the
// CRC (its decode_header / decode_payload are stubs).  This kernel does what an LE sniffer does with a claim: one wave per
// BTGPU_KIND_AA hit, behind header_sweep_kernel on the tail stream, on the packed symbols the two classic sweeps already read.
//
// The CRC-24 (Core Vol 6 Part B 3.1.1: x^24 + x^10 + x^9 + x^6 + x^4 + x^3 + x + 1, every byte LSB first, the register sent from
// position 23 down) is kept in REFLECTED form: bit k of the state is position 23 - k, so the state is shifted right, the
// feedback is 0xDA6000 (bit 23 | 0x5A6000), the advertising init 0x555555 reads 0xAAAAAA, and the 24 CRC symbols packed in air
// order are the state itself.  As a polynomial bit k is the coefficient of x^(23 - k); clocking a zero bit in is a multiplication
// by x mod the polynomial.  The register is linear over GF(2), and that is the design:
//
//   phase A   the record's symbols from offset + 40 on, re-aligned to bit 0, masked to the symbols the record has and XOR-ed with
//             the channel's whitening sequence -- 82 words of LDS, each lane its own words (window index + 32 mod 127 per word).
//   phase B   lane i owns bytes [5 i, 5 i + 5) of header | payload | CRC (64 x 5 = 320 >= 2 + 255 + 3).  Its zero-init CRC c_i
//             (five steps of the byte table) times x^(40 (63 - i)) is its contribution to the register behind byte 320; the
//             XOR prefix of those over the wave (shuffles only) is E_i = S_i x^(40 (64 - i)), and one more multiplication, by
//             x^(-40 (64 - i)), is S_i: the register in front of the lane's chunk for init 0.  Adding init x^(40 i) gives it
//             for any init; for the advertising init that term is a table.  Every lane then walks its five bytes and at every
//             byte boundary m compares the register with the 24 symbols that follow (they may reach into the next lane's chunk):
//             all 256 payload lengths in one pass.  The verdict is the compare at m = 2 + len.  match_len asks of every length L
//             whether the PDU AS IT WOULD BE AT THAT LENGTH -- the header's length byte reading L -- has a CRC that holds: the
//             byte's change d = len ^ L adds crc0(d) x^(8 L) to the register at m = 2 + L, one more multiplication per boundary
//             (nothing at L = len).  The first L that holds (ballot + ctz) is the packet's length also where the length field
//             itself took the bit error, which the plain compare can never find: the CRC covers the header.  The init under which the CRC at the header's length holds is
//                 init = A + (crc_rx + s_m) x^(-8 m)        (s_m: the advertising-init register at m;  A = 0xAAAAAA)
//             -- the register run backwards, possible because the polynomial's constant term is 1.
//
// Conventions of the record (btgpu_le_sweep): symbols the record does not have read as 0 BEFORE dewhitening; a compare counts
// only where all 24 symbols behind the boundary exist; crc_rx is the register image of those 24 symbols (first symbol = bit 0);
// crc_init is in the specification's order (0x555555 on a good advert).  Records that are not computed at all -- kind AC, no
// symbols kept, a channel without an LE index -- are zero with verdict -1, crc_init 0xFFFFFFFF and match_len -1.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "kernels.hip.h"

namespace btgpu {

struct LeRec { uint16_t header; int16_t verdict; int32_t length; uint32_t crc_rx; uint32_t crc_init; int16_t match_len; int16_t pad_; };   // == btgpu_le_sweep
static_assert(sizeof(LeRec) == 20, "five words");

constexpr int kLeWords = 82;                  // 320 bytes of PDU = 80 words, + the two words a lane's 64-symbol view may reach into
constexpr uint32_t kLeFeedback = 0xDA6000u;   // bit 23 | 0x5A6000
constexpr uint32_t kLeAdvInit = 0xAAAAAAu;    // 0x555555, reflected
constexpr uint32_t kLeOne = 0x800000u;        // x^0

constexpr uint32_t le_mulx(uint32_t r) { return (r >> 1) ^ ((r & 1u) ? kLeFeedback : 0u); }                       // r x
constexpr uint32_t le_divx(uint32_t r) { return (r & kLeOne) ? (((r ^ kLeFeedback) << 1) | 1u) : (r << 1); }      // r x^-1
// a b mod the polynomial: Horner over b's coefficients from x^23 (bit 0) down to x^0 (bit 23)
__host__ __device__ constexpr uint32_t le_mulmod(uint32_t a, uint32_t b)
{
    uint32_t r = 0;
    for (int k = 0; k < 24; k++) { r = le_mulx(r); if ((b >> k) & 1u) r ^= a; }
    return r;
}

struct LeSweepTables {
    uint32_t win[127];                // win[k] bit j = whitening bit (k + j) mod 127 (x^7 + x^4 + 1: the classic sequence, other starts)
    uint8_t  start[40];               // where the sequence of LE channel index i begins (position 0 = 1, 1..6 = the index MSB first)
    uint32_t crc[256];                // the register after eight zero bits from state x: x . x^8
    uint32_t pow8[316];               // x^(8 m)
    uint32_t adv40[64];               // 0xAAAAAA x^(40 k): the advertising init carried to the front of lane k's chunk
    uint32_t inv8[321];               // x^(-8 m)
};

constexpr LeSweepTables le_make_tables()
{
    LeSweepTables t{};
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
    for (int c = 0; c < 40; c++) {
        uint8_t r[7] = {1, (uint8_t)((c >> 5) & 1), (uint8_t)((c >> 4) & 1), (uint8_t)((c >> 3) & 1), (uint8_t)((c >> 2) & 1),
                        (uint8_t)((c >> 1) & 1), (uint8_t)(c & 1)};
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
        for (int k = 0; k < 8; k++) r = le_mulx(r);
        t.crc[x] = r;
    }
    uint32_t pw = kLeOne, ad = kLeAdvInit;
    for (int m = 0; m < 316; m++) {
        t.pow8[m] = pw;
        for (int j = 0; j < 8; j++) pw = le_mulx(pw);
    }
    for (int k = 0; k < 64; k++) {
        t.adv40[k] = ad;
        for (int j = 0; j < 40; j++) ad = le_mulx(ad);
    }
    uint32_t iv = kLeOne;
    for (int m = 0; m <= 320; m++) {
        t.inv8[m] = iv;
        for (int j = 0; j < 8; j++) iv = le_divx(iv);
    }
    return t;
}
__device__ const LeSweepTables kLeTables = le_make_tables();
static_assert(le_mulmod(le_make_tables().pow8[315], le_make_tables().inv8[315]) == kLeOne, "x^2520 x^-2520 = 1");

__device__ __forceinline__ uint32_t le_brev24(uint32_t v) { return __brev(v) >> 8; }

// One wave per hit, grid-strided over the hit list like payload_sweep_kernel.  le_index_g: classic channel number -> LE index (or -1),
// the window kernel's table; low_channel + channel_idx is the hit's channel number.
__global__ __launch_bounds__(64) void le_sweep_kernel(
    const DeviceHit *__restrict__ hits, const unsigned int *__restrict__ hit_count, int max_hits,
    const uint32_t *__restrict__ symbits, const int8_t *__restrict__ le_index_g, int low_channel,
    LeRec *__restrict__ out)
{
    __shared__ uint32_t pdu[kLeWords];
    __shared__ uint32_t win[127];
    __shared__ uint32_t crctab[256];
    const int lane = threadIdx.x;
    for (int k = lane; k < 127; k += 64) win[k] = kLeTables.win[k];
    for (int k = lane; k < 256; k += 64) crctab[k] = kLeTables.crc[k];
    const uint32_t up = kLeTables.pow8[5 * (63 - lane)], down = kLeTables.inv8[5 * (64 - lane)], adv = kLeTables.adv40[lane];
    unsigned int n = *hit_count;
    if (n > (unsigned int)max_hits) n = (unsigned int)max_hits;
    for (unsigned int i = blockIdx.x; i < n; i += gridDim.x) {
        const DeviceHit h = hits[i];
        const int ch = low_channel + h.channel_idx;
        const int le_index = (h.kind == 1 && h.sym >= 0 && ch >= 0 && ch < 79) ? (int)le_index_g[ch] : -1;
        if (le_index < 0 || le_index >= 40) {
            if (lane == 0) { LeRec r{}; r.verdict = -1; r.crc_init = 0xffffffffu; r.match_len = -1; out[i] = r; }
            continue;
        }
        int length = h.nsym < 32 * kSymWords - h.offset ? h.nsym : 32 * kSymWords - h.offset;
        length = length < 0 ? 0 : length;
        const int size = length - 40;                    // symbols behind the access address (may be negative)
        const uint32_t *row = symbits + (size_t)h.sym * kSymWords;
        __syncthreads();                                 // (the previous hit's phase B has left the stream)

        // ---------------- phase A: the dewhitened PDU ----------------
        {
            const int p0 = h.offset + 40, w0 = p0 >> 5, sh = p0 & 31;
            const int st = kLeTables.start[le_index];
            for (int k = lane; k < kLeWords; k += 64) {
                uint32_t v = 0;
                if (32 * k < size) {
                    const uint32_t lo = w0 + k < kSymWords ? row[w0 + k] : 0u, hi = w0 + k + 1 < kSymWords ? row[w0 + k + 1] : 0u;
                    v = sh ? (lo >> sh) | (hi << (32 - sh)) : lo;
                    if (size - 32 * k < 32) v &= (1u << (size - 32 * k)) - 1u;   // symbols at positions >= length read as 0
                }
                pdu[k] = v ^ win[(st + 32 * k) % 127];
            }
        }
        __syncthreads();

        // ---------------- phase B: lane = five bytes ----------------
        const uint32_t hdr16 = pdu[0] & 0xffffu;
        const int mh = 2 + (int)(hdr16 >> 8);            // the boundary behind header + payload, by the header's 8-bit length
        uint64_t v;                                      // symbols 40 lane .. + 63: the chunk and the 24 behind its last boundary
        {
            const int q = 40 * lane, w = q >> 5, sh = q & 31;
            v = ((uint64_t)pdu[w + 1] << 32) | pdu[w];
            if (sh) v = (v >> sh) | ((uint64_t)pdu[w + 2] << (64 - sh));
        }
        uint32_t c = 0;
        for (int b = 0; b < 5; b++) c = (c >> 8) ^ crctab[(c ^ (uint32_t)(v >> (8 * b))) & 0xffu];
        uint32_t e = le_mulmod(c, up);
        for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(e, d, 64); if (lane >= d) e ^= o; }
        e = __shfl_up(e, 1, 64);
        if (lane == 0) e = 0;
        uint32_t s = le_mulmod(e, down) ^ adv;           // the advertising-init register in front of byte 5 lane

        int mym = 0x7fff;                                // the lane's first boundary at which the CRC holds
        uint32_t at_rx = 0, at_s = 0;                    // ... and what the boundary of the header's length saw
        for (int b = 0; b < 5; b++) {
            const int m = 5 * lane + b;
            const uint32_t rx = (uint32_t)(v >> (8 * b)) & 0xffffffu;
            if (m == mh) { at_rx = rx; at_s = s; }
            if (m >= 2 && m <= 257 && 8 * m + 24 <= size && mym == 0x7fff) {
                // the hypothesis "the payload is m - 2 bytes long" includes the header's length byte saying so: the CRC of the PDU
                // with that byte put right differs from the one walked here by the byte's change carried m - 2 bytes on
                const uint32_t fix = le_mulmod(crctab[((hdr16 >> 8) ^ (uint32_t)(m - 2)) & 0xffu], kLeTables.pow8[m - 2]);
                if (rx == (s ^ fix)) mym = m;
            }
            s = (s >> 8) ^ crctab[(s ^ rx) & 0xffu];
        }
        const int owner = mh / 5;                        // <= 51
        at_rx = __shfl(at_rx, owner, 64);
        at_s = __shfl(at_s, owner, 64);
        const unsigned long long any = __ballot(mym != 0x7fff);
        const int first = any ? __shfl(mym, __builtin_ctzll(any), 64) : 0x7fff;
        if (lane == 0) {
            LeRec r{};
            r.header = (uint16_t)hdr16;
            r.length = length;
            r.crc_rx = at_rx;
            r.match_len = first == 0x7fff ? (int16_t)-1 : (int16_t)(first - 2);
            if (8 * mh + 24 <= size) {
                r.verdict = at_rx == at_s ? 1 : 0;
                r.crc_init = le_brev24(kLeAdvInit ^ le_mulmod(at_rx ^ at_s, kLeTables.inv8[mh]));
            } else {
                r.verdict = -1;
                r.crc_init = 0xffffffffu;
            }
            out[i] = r;
        }
    }
}

// The records leave for the host as the payload sweeps do: the first min(count, cap) straight into page-locked memory, a word per lane.
__global__ __launch_bounds__(256) void le_out_kernel(const unsigned int *__restrict__ counts, int max_hits,
                                                     const uint32_t *__restrict__ le, uint32_t *__restrict__ h_le, unsigned int cap)
{
    unsigned int n = counts[0];
    n = n > (unsigned int)max_hits ? (unsigned int)max_hits : n;
    const size_t m = (size_t)(n < cap ? n : cap) * (sizeof(LeRec) / 4);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (size_t)gridDim.x * blockDim.x) h_le[i] = le[i];
}

}  // namespace btgpu
