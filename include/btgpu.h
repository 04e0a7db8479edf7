/*
 * btgpu.h -- C ABI of the MI355X-native gr-bluetooth multi-channel sniffer hot path.
 *
 * This is the drop-in boundary: a GNU Radio block (gr::bluetooth::multi_LAP /
 * gr::bluetooth::multi_sniffer, see gr-bluetooth_amd/host/ and INTEGRATION.md) keeps
 * the reference's make()/work() surface and forwards to these entry points.  Plain
 * pointers and sizes only; no C++ or torch types; no exceptions cross this boundary
 * (every function returns BTGPU_OK or a negative BTGPU_E* code).
 *
 * Reference interfaces replaced (paths relative to the gr-bluetooth checkout):
 *   btgpu_design_query   multi_block::multi_block + set_symbol_history + set_channels
 *                        (lib/multi_block.cc:40-120, :299-342): pure host arithmetic
 *   btgpu_create         multi_LAP::make / multi_sniffer::make
 *                        (lib/multi_LAP_impl.cc:39-56, lib/multi_sniffer_impl.cc:42-72)
 *   btgpu_work           multi_LAP_impl::work / multi_sniffer_impl::work
 *                        (lib/multi_LAP_impl.cc:65-114, lib/multi_sniffer_impl.cc:82-166):
 *                        same input contract (history()-1 old items followed by the new
 *                        ones), but consumes every whole slot in the buffer at once
 *   btgpu_process_device same work on a device-resident stream segment (time-partitioned
 *                        multi-GPU and bench entry; no reference counterpart)
 *   btgpu_process_host   ... on a host-resident segment (what btrx_amd --gpus N gives each device)
 *   btgpu_poll           replaces the printf side effect of work(): hit records in the
 *                        order the reference's loops print them (slot, channel, offset)
 *   btgpu_acgen          classic_packet::acgen (lib/packet_impl.cc:309-364)
 */
#ifndef BTGPU_H
#define BTGPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BTGPU_OK            0
#define BTGPU_EINVAL       -1   /* bad argument / unsupported configuration */
#define BTGPU_ENOMEM       -2
#define BTGPU_EDEVICE      -3   /* HIP runtime error (see btgpu_last_error)  */
#define BTGPU_ENODEVICE    -4   /* no gfx950 device visible                  */
#define BTGPU_EOVERFLOW    -5   /* hit buffer overflow (hits were dropped)   */
#define BTGPU_EUNSUPPORTED -6

#define BTGPU_MODE_LAP      0   /* gr::bluetooth::multi_LAP     (+68 symbols of history)   */
#define BTGPU_MODE_SNIFFER  1   /* gr::bluetooth::multi_sniffer (+3125 symbols of history) */

#define BTGPU_CHANNELIZER_AUTO      0
#define BTGPU_CHANNELIZER_DIRECT    1   /* per-channel direct-form DDC; bit-exact vs the oracle */
#define BTGPU_CHANNELIZER_POLYPHASE 2   /* polyphase filter bank; equal within float tolerance   */

#define BTGPU_SQUELCH_AUTO      0
#define BTGPU_SQUELCH_DIRECT    1       /* exact direct-form 20001-tap-class noise DDC           */
#define BTGPU_SQUELCH_STAGED    2       /* two-stage equivalent filter + quadrature (tolerance)  */

#define BTGPU_CORRELATOR_AUTO   0       /* multi_LAP: BTBB (what the reference links), multi_sniffer: INTREE */
#define BTGPU_CORRELATOR_INTREE 1       /* classic_packet::sniff_ac / check_ac (lib/packet_impl.cc:247-268,471-510) */
#define BTGPU_CORRELATOR_BTBB   2       /* libbtbb btbb_find_ac with btbb_init(1), max_ac_errors 1, LAP_ANY
                                           (lib/multi_LAP_impl.cc:55,93) [EXT libbtbb, unpinned]; multi_LAP
                                           only; hit.offset is then the sync-word start and hit.ac_errors the
                                           number of corrected bits (0 or 1)                            */

#define BTGPU_FLAG_LE        0x1        /* also run the le_packet::sniff_aa pass (sniffer mode)  */
#define BTGPU_FLAG_DEBUG_Y   0x2        /* keep the channel-bank output Y for btgpu_debug_fetch  */
#define BTGPU_FLAG_SYMBOLS   0x8        /* keep the sliced symbols of every window that reported a
                                           hit; fetch them with btgpu_poll_symbols                */
#define BTGPU_FLAG_HEADERS   0x10       /* (implies SYMBOLS) sweep the packet header of every classic hit
                                           over the 64 CLK1-6 candidates on the GPU; btgpu_poll_headers   */
#define BTGPU_FLAG_ASYNC     0x4        /* work/process_device return once a batch is enqueued;
                                           its records appear in a later btgpu_poll (always in
                                           stream order) or after btgpu_flush.  The tail of batch
                                           n (finish_kernel, record copy) overlaps batch n+1.    */

#define BTGPU_FLAG_TIMING    0x20       /* bracket the kernels of every batch with HIP events for btgpu_last_timing
                                           (off by default: eleven event records per batch are not free)     */
#define BTGPU_FLAG_TIMING_BANK 0x80      /* the light form: events only around the channel-bank kernel (BTGPU_K_DDC_CHANNEL) and the exact
                                           rows' kernel (BTGPU_K_EXACT); what bench.py's timed region uses for its roofline figures */
#define BTGPU_FLAG_NO_NSYM   0x40       /* LAP-list consumers (multi_LAP prints the LAP only, lib/multi_LAP_impl.cc:93-110):
                                           skip the clock-recovery continuation over the rest of a hit window that
                                           only produces hit.nsym; nsym is then -1 unless the window ended inside
                                           the 693-symbol detection span.  Ignored with BTGPU_FLAG_SYMBOLS / HEADERS */

#define BTGPU_FLAG_NO_VERIFY 0x100      /* polyphase channelizer only: do NOT recompute the demodulated rows of the busy windows (energy
                                           anywhere in the detection span: "presence") through the bit-exact direct-form arithmetic.  By
                                           default they are (exact rows, DESIGN.md sections 4.4 and 5): the records then equal the CPU
                                           reference's in slot, channel, kind, offset, LAP and ac_errors, and the symbols handed to the
                                           host layer are the reference's to the end of each packet; with this flag ~1e-4 .. 2e-2 of the
                                           records (by traffic) come out a symbol apart or on one side only (the round-3 behaviour).
                                           Exact rows are served at every rate the polyphase channelizer is: 4 .. 100 Msps, even */

#define BTGPU_FLAG_EXACT_PAYLOAD 0x200   /* accepted; ALWAYS ON since round 6.  The symbols a record hands to the host layer are the reference's
                                           own arithmetic to the END OF THE PACKET: a packet's air time is busy, so its rows are exact rows
                                           anyway (no separate pass).  What every payload decode and CRC of the host layer sees
                                           (lib/packet_impl.cc:1066-1160) equals the CPU reference's */

#define BTGPU_FLAG_EXACT_ALL 0x400       /* polyphase channelizer: NO SELECTION AT ALL -- every row of every channel is recomputed by the reference's
                                           direct-form arithmetic on the matrix pipe (presence marks everything): every field of every record,
                                           nsym and the records born from noise included, equals the CPU reference's with the bit-exact
                                           channelizer's (the squelch figure stays the staged filter's: SNR within 3.4e-6 dB).  ~8 Gsamples/s
                                           at 79 channels / 100 Msps instead of ~30.  Honoured at every rate the
                                           polyphase channelizer serves: 4 .. 100 Msps, even (52 .. 98 in the dense form only) */

#define BTGPU_FLAG_EXACT_DENSE 0x800     /* exact rows in their DENSE form (csrc/exact_dense.hip.h: 16 channels per matrix row block, the decimation a
                                           run-time argument) also where the tile-sparse form exists.  The same bits in every row either way; the
                                           dense form is what runs at 52 .. 64 Msps, where the sparse one is not instantiated.  The environment's
                                           BTGPU_EXACT_FORM=dense | sparse does the same for A/B timing (profiles/exact_dense_ab.json) */

#define BTGPU_FLAG_DIRECT_MFMA 0x1000    /* the direct-form banks (DIRECT channelizer, DIRECT squelch, the segmented rates: odd and fractional
                                           samples per symbol) on the matrix pipe (csrc/ddc_mfma.hip.h) instead of the vector ALU.  The same
                                           bits in every output either way; BTGPU_DIRECT_FORM=mfma | valu in the environment does the same
                                           (profiles/direct_mfma_ab.json).  The staged squelch's direct stage 1 stays on the vector ALU */

#define BTGPU_FLAG_PAYLOAD_SWEEP 0x2000   /* (implies HEADERS) behind the header sweep, classic_packet::crc_check under the same 64 CLK1-6 candidates
                                           on the GPU (csrc/payload_sweep.hip.h): FEC 2/3, unwhitening, payload header, CRC-16 -- the other
                                           half of what basic_rate_piconet::UAP_from_header asks of a packet; btgpu_poll_payloads.  Sniffer
                                           mode only (multi_LAP has no packet handlers: BTGPU_EUNSUPPORTED from btgpu_design_query and
                                           btgpu_create).  Without the flag nothing of it is allocated or launched */

#define BTGPU_FLAG_EXACT_NARROW 0x4000    /* exact rows in their NARROW form (csrc/exact_narrow.hip.h: eight channels x (re, im) as the 16 rows of
                                           v_mfma_f32_16x16x4_f32, the row block's taps resident in registers).  The same bits in every row as
                                           the other forms.  Exists on the polyphase channelizer with decimation <= 8 (the even rates
                                           4 .. 16 Msps); with the flag at a higher rate or with a DIRECT channelizer btgpu_design_query and
                                           btgpu_create return BTGPU_EUNSUPPORTED.  BTGPU_EXACT_FORM=narrow in the environment asks for it
                                           where it exists and is ignored elsewhere (A/B timing: profiles/exact_narrow_ab.json) */

#define BTGPU_FLAG_LE_SWEEP 0x8000        /* (implies SYMBOLS; needs BTGPU_FLAG_LE, sniffer mode) behind every access-address hit, on the GPU
                                           (csrc/le_sweep.hip.h): the dewhitened PDU header, the CRC-24 at the header's length and at every
                                           other payload length, and the CRCInit the packet implies; btgpu_poll_le.  Without BTGPU_FLAG_LE or
                                           in BTGPU_MODE_LAP: BTGPU_EUNSUPPORTED from btgpu_design_query and btgpu_create.  Without the flag
                                           nothing of it is allocated or launched */

#define BTGPU_KIND_AC 0
#define BTGPU_KIND_AA 1

typedef struct btgpu_handle btgpu_handle;

typedef struct btgpu_config {
    double  sample_rate;      /* multi_*::make(sample_rate, ...)            */
    double  center_freq;      /* multi_*::make(..., center_freq, ...)       */
    double  squelch_db;       /* multi_*::make(..., squelch_threshold)      */
    int32_t mode;             /* BTGPU_MODE_*                               */
    int32_t device;           /* HIP device ordinal, -1 = current device    */
    int32_t channelizer;      /* BTGPU_CHANNELIZER_*                        */
    int32_t squelch;          /* BTGPU_SQUELCH_*                            */
    int32_t flags;            /* BTGPU_FLAG_*                               */
    int32_t max_batch_slots;  /* slots per internal batch, 0 = default      */
    int32_t max_hits;         /* hit-buffer capacity per batch, 0 = default */
    int32_t correlator;       /* BTGPU_CORRELATOR_*                          */
} btgpu_config;

/* Everything the multi_block constructor derives (lib/multi_block.cc:56-119). */
typedef struct btgpu_design {
    double  samples_per_symbol;
    int32_t samples_per_slot;
    int32_t decimation;
    int32_t ntaps_channel, ntaps_noise;
    int32_t low_channel, high_channel;       /* classic channel numbers, inclusive */
    int32_t first_channel_sample, first_noise_sample;
    int32_t history;                          /* history() incl. symbol history     */
    int32_t ddc_out;                          /* channel DDC outputs per window     */
    int32_t noise_out;                        /* noise DDC outputs per window       */
    int32_t channelizer;                      /* resolved BTGPU_CHANNELIZER_*       */
    int32_t squelch;                          /* resolved BTGPU_SQUELCH_*           */
    int32_t left_margin;                      /* samples before a device segment the staged
                                                 squelch may read (0 for DIRECT)     */
    int32_t correlator;                       /* resolved BTGPU_CORRELATOR_*        */
} btgpu_design;

typedef struct btgpu_hit {
    uint64_t slot;        /* work() call index == "time slot" the reference prints          */
    int32_t  channel;     /* classic channel 0..78                                          */
    int32_t  offset;      /* symbol offset in the window's symbol array (sniff_ac result)    */
    uint32_t lap;         /* LAP (kind AC) / access address (kind AA)                       */
    int32_t  ac_errors;   /* mismatches over the 68 checked access-code bits               */
    int32_t  kind;        /* BTGPU_KIND_*                                                   */
    int32_t  nsym;        /* symbols available to the packet handler from `offset` on       */
    double   snr_db;      /* 10 log10(E_on / E_off) of the (slot, channel) window           */
} btgpu_hit;

/* Per-kernel GPU time (needs BTGPU_FLAG_TIMING; zeros otherwise), cumulative since btgpu_create (callers take
 * differences), measured with HIP events recorded on the streams the kernels are launched on; a batch is
 * accounted when its records are harvested.  With BTGPU_FLAG_ASYNC up to three batches are in flight (banks of
 * batch n+2, post stage of n+1, tail of n on three streams): a kernel's time then includes what it loses to
 * the kernels running beside it. */
#define BTGPU_K_DDC_CHANNEL   0   /* channel bank (direct DDC or polyphase channelizer) */
#define BTGPU_K_DEMOD_ENERGY  1   /* direct form: quadrature demod + |Y|^2 block sums; polyphase: tile sums -> block sums */
#define BTGPU_K_DDC_NOISE     2   /* noise bank                                          */
#define BTGPU_K_NOISE_ENERGY  3   /* noise |Y|^2 per-slot sums                           */
#define BTGPU_K_WINDOW        4   /* squelch + M&M + slicer + access-code search         */
#define BTGPU_K_FINISH        5   /* M&M continuation of the windows that reported hits  */
#define BTGPU_K_VERIFY        6   /* the second run (tail stream): exact rows under the first run's uncovered hits, fill, window kernel over those windows */
#define BTGPU_K_EXACT         7   /* exact_rows_kernel over presence's marks, in line before the window kernel (bracketed with BTGPU_FLAG_TIMING_BANK too) */
#define BTGPU_K_COUNT         8
typedef struct btgpu_timing {
    float    kernel_ms[BTGPU_K_COUNT];        /* summed over launches                  */
    uint32_t kernel_launches[BTGPU_K_COUNT];
    float    total_ms;                        /* first kernel start to last kernel end */
    uint32_t batches;
    uint64_t samples;                         /* new complex samples consumed          */
    uint64_t slots;
    uint64_t verify_windows;                  /* busy windows (presence) + windows of the second run (always counted)    */
    uint64_t verify_rows;                     /* demodulated rows recomputed by exact_rows_kernel (both launches), in tiles of 1250 / 11 rows */
    uint64_t verify_turned_away;              /* windows that should have gone to the second run but found its list full */
    uint64_t long_tasks;                      /* windows of the second run (a classic hit on rows presence had not covered) */
    uint64_t long_rows;                       /* ... the rows recomputed for them                                         */
    uint64_t long_turned_away;                /* (unused since round 6)                                                   */
} btgpu_timing;

/* ---- host-only helpers (no GPU needed) ---- */
int  btgpu_design_query(const btgpu_config *cfg, btgpu_design *out);
int  btgpu_acgen(uint32_t lap, uint8_t ac[9]);
int  btgpu_filter_taps(const btgpu_config *cfg, int which /*0 channel, 1 noise*/, float *taps, int cap);
const char *btgpu_strerror(int code);
const char *btgpu_version(void);

/* ---- block lifetime ---- */
int  btgpu_create(const btgpu_config *cfg, btgpu_handle **out);
void btgpu_destroy(btgpu_handle *h);          /* frees the handle's memory; its eight HIP streams are kept by the library and handed
                                                 to the next btgpu_create on the same device (streams created after others were
                                                 destroyed measured 25 % slower steps; BTGPU_STREAM_POOL=0 in the environment: off) */
int  btgpu_get_design(const btgpu_handle *h, btgpu_design *out);
int  btgpu_history(const btgpu_handle *h);
int  btgpu_device(const btgpu_handle *h);     /* HIP ordinal the handle lives on (what device = -1 resolved to) */
int  btgpu_device_count(void);                /* visible HIP devices (whatever their architecture: btgpu_create checks
                                                 for gfx950), or BTGPU_ENODEVICE                                  */
const char *btgpu_last_error(const btgpu_handle *h);

/* ---- work() ----
 * `items` is what GNU Radio hands to work(): interleaved float32 I/Q, history()-1 old
 * samples followed by the new ones, `n_items` complex samples in total (so GNU Radio's
 * noutput_items = n_items - (history()-1)).  Processes S = noutput_items / samples_per_slot
 * whole slots -- the reference processes exactly one per call and returns samples_per_slot
 * (lib/multi_sniffer_impl.cc:165); S consecutive reference calls give the same records --
 * queues their hits, stores S*samples_per_slot in *consumed.  Returns BTGPU_OK or <0. */
int btgpu_work(btgpu_handle *h, const float *items, size_t n_items, size_t *consumed);

/* Streaming convenience: keeps history internally (zero pre-filled like the GNU Radio
 * scheduler) so arbitrary chunks can be pushed.  Float input only: the history it carries is float32 (there is no
 * btgpu_push_s16; an int16 source widens its chunks or calls btgpu_work_s16 on its own buffer). */
int btgpu_push(btgpu_handle *h, const float *iq, size_t n_complex);

/* Device-resident segment: d_iq[left_margin] is absolute sample
 * first_slot*samples_per_slot-(history()-1); from there the segment must hold
 * history() + (n_slots-1)*samples_per_slot complex samples.  The `left_margin` samples in
 * front (real stream data when the segment is cut out of a longer stream; 0 at the stream
 * start, where GNU Radio's pre-filled zeros are implied) let the staged squelch filter see
 * the same samples the reference's noise filter would; btgpu_design.left_margin is enough.
 * `hip_stream` is a hipStream_t (NULL = the handle's own stream).  The segment must stay valid until the
 * batch's records have been handed out (btgpu_flush, or a btgpu_poll that returns them): the exact
 * confirmation of the polyphase path re-reads the samples of the windows it takes on the handle's tail stream. */
int btgpu_process_device(btgpu_handle *h, const void *d_iq, size_t n_complex, size_t left_margin,
                         uint64_t first_slot, uint64_t n_slots, void *hip_stream);

/* The same for a segment in HOST memory (one rank of a time-partitioned run driven from C/C++): the library
 * stages it batch by batch through two pinned buffers, the copy of one batch overlapping the kernels of the
 * previous one (with BTGPU_FLAG_ASYNC).  Same layout and meaning of the arguments as btgpu_process_device. */
int btgpu_process_host(btgpu_handle *h, const float *iq, size_t n_complex, size_t left_margin,
                       uint64_t first_slot, uint64_t n_slots);

/* ---- complex int16 input (what the SDRs put on the wire; the reference's `btrx -s` / interleaved_short_to_complex) ----
 * The three entries above for interleaved int16 I/Q, argument for argument: sizes, margins and slots stay in COMPLEX samples
 * (one sample = two int16 = 4 bytes).  The samples travel to the device as they are -- half the bytes of the float entries --
 * and are widened inside the kernels at their input loads with (float)int16, NO scale factor and no DC correction: int16 ->
 * float32 is exact, so every record, the demodulated stream and the window energies are bit for bit what the float entry
 * returns for the same values.  Every configuration btgpu_create accepts takes either format, and a handle may be fed
 * either format from call to call (the margin btgpu_work carries between calls is kept as float32; an int16 call that
 * follows a float call rounds those few samples to int16, saturating).
 * Alignment: the kernels load int16 samples in aligned pairs, so the device pointer given to btgpu_process_device_s16 must
 * be 8-byte aligned (BTGPU_EINVAL otherwise); host pointers need only the int16's own 2 bytes (they are staged into buffers
 * of the library's own). */
int btgpu_work_s16(btgpu_handle *h, const int16_t *items, size_t n_items, size_t *consumed);
int btgpu_process_host_s16(btgpu_handle *h, const int16_t *iq, size_t n_complex, size_t left_margin,
                           uint64_t first_slot, uint64_t n_slots);
int btgpu_process_device_s16(btgpu_handle *h, const void *d_iq, size_t n_complex, size_t left_margin,
                             uint64_t first_slot, uint64_t n_slots, void *hip_stream);

/* ---- complex int8 input (the 8-bit wire formats: USRP sc8, bladeRF 2.0's 8-bit mode, HackRF) ----
 * The same three entries for interleaved int8 I/Q, argument for argument: re in the low byte, im in the next, one complex
 * sample = 2 bytes; sizes, margins and slots stay in COMPLEX samples.  The samples travel to the device as they are -- a
 * quarter of the float entries' bytes -- and are widened inside the kernels at their input loads with (float)int8, NO scale
 * factor and no DC correction: exact, so records, demodulated stream and window energies are bit for bit the float entry's
 * for the same values.  Every configuration btgpu_create accepts takes this format, and a handle may be fed float, int16 or
 * int8 from call to call (the margin btgpu_work carries stays float32; an int8 call that follows a wider one rounds those few
 * samples to int8, saturating at -128 / 127).
 * Alignment: the widest load the kernels issue on an int8 stream is one aligned 32-bit word (two samples), so the device
 * pointer given to btgpu_process_device_s8 must be 4-byte aligned (BTGPU_EINVAL otherwise); host pointers need 1 byte (they
 * are staged into buffers of the library's own).  btgpu_push stays float-only. */
int btgpu_work_s8(btgpu_handle *h, const int8_t *items, size_t n_items, size_t *consumed);
int btgpu_process_host_s8(btgpu_handle *h, const int8_t *iq, size_t n_complex, size_t left_margin,
                          uint64_t first_slot, uint64_t n_slots);
int btgpu_process_device_s8(btgpu_handle *h, const void *d_iq, size_t n_complex, size_t left_margin,
                            uint64_t first_slot, uint64_t n_slots, void *hip_stream);

/* Drain queued hits, ordered by (slot, channel, kind, offset). Returns count (>=0) or <0. */
int btgpu_poll(btgpu_handle *h, btgpu_hit *out, int max_hits);
/* Like btgpu_poll, plus what the reference hands to its packet handlers with every hit
 * (lib/multi_sniffer_impl.cc:116: ac(&symp[i], len - i, ...)): the window's sliced symbols from the
 * hit offset on, one symbol per byte (air order), up to sym_cap per hit, written to
 * symbols[i*sym_cap ...]; sym_len[i] = number written (min(nsym, sym_cap)).  Needs
 * BTGPU_FLAG_SYMBOLS; note the LE quirk Q6: for kind AA nsym counts from the reduced length. */
int btgpu_poll_symbols(btgpu_handle *h, btgpu_hit *out, uint8_t *symbols, int sym_cap, int *sym_len, int max_hits);
/* What classic_packet::try_clock(clock) yields for clock = 0..63 (lib/packet_impl.cc:1046-1063): the UAP
 * that satisfies the HEC and the packet type, from the FEC-1/3-decoded, unwhitened header; fec13_ok = 0
 * where unfec13 (:367-383) reports failure (try_clock then returns 0 and leaves type/UAP alone). */
typedef struct btgpu_header {
    uint8_t uap[64];
    uint8_t type[64];
    int32_t fec13_ok;
    int32_t reserved;
} btgpu_header;
/* btgpu_poll_symbols plus the header sweep of each record (zeroed for kind AA); needs BTGPU_FLAG_HEADERS */
int btgpu_poll_headers(btgpu_handle *h, btgpu_hit *out, btgpu_header *hdr, uint8_t *symbols, int sym_cap,
                       int *sym_len, int max_hits);
/* What classic_packet::crc_check(clock) returns right after try_clock(clock) on a fresh packet, for clock = 0..63
 * (lib/packet_impl.cc:612-671): 0 refuted (FHS, DM1 and HV1 only), 1 inconclusive, 10 CRC correct, 1000 FHS CRC correct; -1 = not
 * computed (fec13_ok = 0 -- try_clock fails, crc_check is never asked -- and kind AA).  Type and UAP are the header sweep's for the
 * same clock.  `length` is the number of symbols from hit.offset on that the verdicts were computed on: min(nsym, 3840 - offset), the
 * packed symbols the device keeps per hit window (symbols beyond it read as 0).  The length guards of crc_check depend on it: a
 * host layer that hands its packet another number of symbols must compute its own verdicts (host/classic.cc does). */
typedef struct btgpu_crc_sweep {
    int16_t verdict[64];
    int32_t length;
    int32_t reserved;
} btgpu_crc_sweep;
/* btgpu_poll_headers plus the payload sweep of each record; needs BTGPU_FLAG_PAYLOAD_SWEEP (BTGPU_EUNSUPPORTED without) */
int btgpu_poll_payloads(btgpu_handle *h, btgpu_hit *out, btgpu_header *hdr, btgpu_crc_sweep *crc, uint8_t *symbols, int sym_cap,
                        int *sym_len, int max_hits);
/* What lies behind an access-address hit (csrc/le_sweep.hip.h).  The PDU is the symbols from hit.offset + 40 on, symbols the record
 * does not have read as 0, dewhitened with the channel's sequence.  header: its first 16 bits, host order; the length field is
 * header >> 8, all eight bits (Core 4.2+).  verdict: 1 the advertising-init (0x555555) CRC-24 over the 2 + len bytes equals the 24
 * symbols that follow, 0 it does not, -1 not computed (kind AC, or fewer than 8 (2 + len + 3) symbols behind the access address).
 * crc_rx: those 24 symbols as the CRC register holds them when it is shifted out (first symbol = bit 0).  crc_init: the init under
 * which the CRC at the header's length holds -- 0x555555 on a good advertising packet, the connection's CRCInit on a data-channel
 * packet; 0xFFFFFFFF where the verdict is -1.  match_len: the smallest payload length L in 0 .. 255 at which the advertising-init
 * CRC of the PDU as it would be at that length -- 2 + L bytes, the header's length byte reading L -- equals the 24 symbols behind
 * it, all of them present; -1 = none.  It is the header's length on a good packet, and the packet's length where the length field
 * itself took the bit error (the CRC covers the header, so the CRC of the PDU as received holds at no length then).  length as in
 * btgpu_crc_sweep.  Records of kind AC are zero with
 * verdict -1, crc_init 0xFFFFFFFF and match_len -1. */
typedef struct btgpu_le_sweep {
    uint16_t header;
    int16_t  verdict;
    int32_t  length;
    uint32_t crc_rx;
    uint32_t crc_init;
    int16_t  match_len;
    int16_t  reserved;
} btgpu_le_sweep;
/* btgpu_poll_symbols plus the LE sweep of each record; needs BTGPU_FLAG_LE_SWEEP (BTGPU_EUNSUPPORTED without) */
int btgpu_poll_le(btgpu_handle *h, btgpu_hit *out, btgpu_le_sweep *le, uint8_t *symbols, int sym_cap, int *sym_len, int max_hits);
/* btgpu_poll_symbols plus whichever sweeps the caller names (hdr, crc, le: each may be null): for a consumer that wants the classic
 * sweeps and the LE sweep of one record stream.  BTGPU_EUNSUPPORTED where a named sweep's flag is off */
int btgpu_poll_records(btgpu_handle *h, btgpu_hit *out, btgpu_header *hdr, btgpu_crc_sweep *crc, btgpu_le_sweep *le, uint8_t *symbols,
                       int sym_cap, int *sym_len, int max_hits);
int btgpu_pending(const btgpu_handle *h);
/* Wait for every enqueued batch and move its records to the poll queue (BTGPU_FLAG_ASYNC). */
int btgpu_flush(btgpu_handle *h);

int btgpu_last_timing(const btgpu_handle *h, btgpu_timing *out);

/* Which form of the exact rows' kernel the handle runs (BTGPU_FLAG_EXACT_DENSE, BTGPU_FLAG_EXACT_NARROW). */
#define BTGPU_EXACT_NONE   0   /* no exact rows: DIRECT channelizer, or BTGPU_FLAG_NO_VERIFY */
#define BTGPU_EXACT_SPARSE 1   /* exact_rows_kernel<D>: one (channel, tile) pair at a time    */
#define BTGPU_EXACT_DENSE  2   /* exact_dense_kernel: channels as the matrix rows             */
#define BTGPU_EXACT_NARROW 3   /* exact_narrow_kernel: eight channels as 16x16x4 matrix rows  */
int btgpu_exact_form(const btgpu_handle *h);

/* Which kernel the handle's direct-form banks run (BTGPU_FLAG_DIRECT_MFMA); VALU also where it has none. */
#define BTGPU_DIRECT_VALU 0    /* ddc_direct_kernel: one lane per output on the vector ALU    */
#define BTGPU_DIRECT_MFMA 1    /* ddc_mfma_kernel: channels as the matrix rows                */
int btgpu_direct_form(const btgpu_handle *h);

/* ---- introspection for parity tests: copies an intermediate of the LAST batch ----
 * what: 0 channel-bank output Y (complex64 [channel][g]; DIRECT channelizer or BTGPU_FLAG_DEBUG_Y),
 *       1 demodulated stream d (float32, time-major [g][nch]: pass channel to get a strided copy),
 *       2 E_on per window (float64, [slot][channel]), 3 E_off per window, 4 snr per window,
 *       5 noise-bank output (complex64; DIRECT squelch only),
 *       10 the exact stage's tasks ({int32 window = slot * nch + channel index, int32 rows, float64 snr}), 11 their exact
 *       demodulated rows (float32 [task][1416]; rows 1 .. rows-1 of a task are valid).
 * channel is a classic channel number (ignored for 2..4); returns elements copied. */
long btgpu_debug_fetch(btgpu_handle *h, int what, int channel, size_t first, size_t count, void *out);

/* Host-side copies of the integer tables the kernels use (header-byte distance tables of
 * le_packet::sniff_aa under the reference's names, "derived/classic_first18", "derived/le_whiten16"):
 * returns bytes written or <0.  For the digest test against the reference's literals. */
int btgpu_debug_lut(const char *name, void *out, int cap_bytes);

/* ---- parity entry: the access-code search on a captured SYMBOL stream ----
 * Runs the window kernel's search (classic_packet::sniff_ac + check_ac, lib/packet_impl.cc:247-268,
 * :471-510) straight on `n` sliced symbols, one per byte (0/1) -- the format of the reference's
 * samples/channel37.dem -- without the float front end.  policy 0: every qualifying offset;
 * policy 1: a stream scan that moves on by 68 symbols after a hit (the sniffer's loop,
 * lib/multi_sniffer_impl.cc:107-127, applied to the whole stream).  Records: offset = absolute
 * symbol offset, lap, ac_errors, nsym = n - offset; ordered by offset.  Returns the number of
 * records (the first `cap` are written) or a negative error.  No handle needed. */
long btgpu_debug_scan_symbols(const uint8_t *symbols, size_t n, int device, int policy, btgpu_hit *out, long cap);

/* ---- parity entry: the two sweeps on captured packets ----
 * `n_packets` symbol arrays, one symbol per byte (0/1), packet i at symbols[i * stride] with lengths[i] (<= stride, <= 3840)
 * symbols from the access-code offset on: the preamble with to_header = 72 (the in-tree correlator's offset), the sync word with
 * to_header = 68 (libbtbb's).  Packs them, runs header_sweep_kernel and payload_sweep_kernel on them as the tail of a batch does
 * (offset 0, nsym = lengths[i]) and returns both records per packet.  Returns n_packets or a negative error.  No handle needed. */
long btgpu_debug_payload_sweep(const uint8_t *symbols, const int32_t *lengths, int n_packets, int stride, int device, int to_header,
                               btgpu_header *hdr, btgpu_crc_sweep *crc);

/* ---- parity entry: the LE sweep on captured packets ----
 * Packet i at symbols[i * stride], one symbol per byte (0/1), from the preamble on (the offset sniff_aa returns), lengths[i]
 * (<= stride, <= 3840) symbols, LE channel index le_index[i] in 0 .. 39.  Runs le_sweep_kernel on them as the tail of a batch does
 * (offset 0, nsym = lengths[i]).  Returns n_packets or a negative error.  No handle needed. */
long btgpu_debug_le_sweep(const uint8_t *symbols, const int32_t *lengths, const int32_t *le_index, int n_packets, int stride,
                          int device, btgpu_le_sweep *out);

/* ---- hop reversal: the piconet's complete hopping sequence on the GPU ----
 * Replaces basic_rate_piconet_impl::init_hop_reversal's precalc + address_precalc + gen_hops
 * (lib/piconet_impl.cc:96-255: a 128 MiB table, one entry per 625 us slot, index = CLK27..1),
 * init_candidates (:285-302), winnow(offset, channel) (:305-321) and hop(clock) (:279-282).
 * address = (UAP << 24 | LAP) & 0xfffffff; afh = the piconet's d_afh flag. */
typedef struct btgpu_hopseq btgpu_hopseq;
int  btgpu_hopseq_create(uint32_t address, int afh, int device, btgpu_hopseq **out);
void btgpu_hopseq_destroy(btgpu_hopseq *h);
/* candidate CLK1-27 values whose hop matches `channel` among those with the known CLK1-6 bits;
 * returns the number of candidates (or a negative error) */
int  btgpu_hopseq_init_candidates(btgpu_hopseq *h, int channel, int known_clock_bits, int aliased);
/* keep the candidates whose hop `offset` slots later is `channel`; returns how many remain */
int  btgpu_hopseq_winnow(btgpu_hopseq *h, int offset, int channel, int aliased);
/* the surviving candidates in ascending order (up to cap); returns their total number */
int  btgpu_hopseq_candidates(btgpu_hopseq *h, uint32_t *out, int cap);
int  btgpu_hopseq_lookup(btgpu_hopseq *h, const uint32_t *index, int n, uint8_t *channel);
long btgpu_hopseq_fetch(btgpu_hopseq *h, size_t first, size_t count, uint8_t *out);   /* table slice */

#ifdef __cplusplus
}
#endif
#endif /* BTGPU_H */
