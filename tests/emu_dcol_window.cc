// The window kernel's two staging forms side by side under the HIP emulator (tests/test_emu_dcol_window.py builds and loads
// this translation unit; emu_bank.cc is included for its set-up): the 100-bin bank writes the demodulated stream in both
// layouts, then window_kernel runs once on the time-major d (WinLayout<3, 96, 20>) and once on the tile-blocked dcol
// (WinLayoutTiled).  Everything the kernel leaves must be the same bytes.
#include "emu/emu_bank.cc"

namespace {
struct WindowOut {
    std::vector<int> win_len, win_fin;
    std::vector<DeviceHit> hits;
    std::vector<FinishRec> fin;
    std::vector<uint32_t> symbits, winbits;
    unsigned int counts[2] = {0, 0};
};

template <class LAY>
void run_window(const Design &des, const WindowParams &p, int S, int nch, const float *stream, long long G, const double *P,
                const double *Pt, const double *Qn, WindowOut &o)
{
    const size_t W = (size_t)S * nch;
    std::vector<double> e_on(W), e_off(W), snr(W);
    o.win_len.assign(W, -1); o.win_fin.assign(W, -1);
    o.hits.assign((size_t)p.max_hits, DeviceHit{});
    o.fin.assign(W, FinishRec{});
    o.symbits.assign(W * kSymWords, 0u);
    o.winbits.assign((size_t)((S + 2) / 3 + 1) * kBitWords * kWinThreads, 0u);
    emu::launch(dim3((unsigned)((S + LAY::kSlots - 1) / LAY::kSlots)), dim3(kWinThreads), [&]() {
        window_kernel<LAY>(p, stream, G, P, Pt, Qn, des.mmse, &des.ac.byte_lo[0][0], &des.ac.byte_hi[0][0], e_on.data(), e_off.data(),
                           snr.data(), o.win_len.data(), o.hits.data(), &o.counts[0], o.fin.data(), &o.counts[1], &des.le.hdr[0][0],
                           des.le.whiten16, des.le.index_of_channel, o.win_fin.data(), o.symbits.data(), o.winbits.data());
    });
}

template <class T>
bool same_bytes(const std::vector<T> &a, const std::vector<T> &b, size_t n)
{
    return a.size() >= n && b.size() >= n && (n == 0 || std::memcmp(a.data(), b.data(), n * sizeof(T)) == 0);
}
}  // namespace

// iq: interleaved complex64 at 100 Msps, S slots; mode: BTGPU_MODE_*.  Returns the number of hits (both runs agree on everything) or a negative code:
// -1 win_len, -2 hit count, -3 hits, -4 fin count, -5 fin records, -6 packed symbols, -7 window -> symbol slot, -8 sliced words;
// <= -100: set-up.  counts_out: hits, fin records.
extern "C" int emu_dcol_window_ab(double fs, double fc, int mode, int le, double squelch_db, const float *iq, long long x_len, int S, int *counts_out)
{
    btgpu_config cfg{};
    cfg.sample_rate = fs; cfg.center_freq = fc; cfg.squelch_db = squelch_db; cfg.mode = mode;
    cfg.flags = le ? BTGPU_FLAG_LE : 0;
    static Design des; static FastPath fp;
    des = Design();
    int rc = make_design(cfg, des);
    if (rc) return -100 + (rc < 0 ? 0 : -1);
    rc = make_fast_path(des, fp);
    if (rc || !fp.channel.available || fp.channel.M != kPfbM) return -102;
    long long sizes[8] = {0};
    rc = emu_bank_run(fs, fc, cfg.mode, iq, x_len, 0, S, 1, nullptr, nullptr, nullptr, nullptr, nullptr, sizes);
    if (rc) return -103;
    const long long G = sizes[0], zstride = sizes[3];
    const int nb = (int)sizes[1], nch = (int)sizes[2];
    std::vector<float4> dbuf(((size_t)(G + 64) * 80 + 3) / 4 + 4);
    float *d = (float *)dbuf.data();
    std::vector<double> P((size_t)nch * nb), Pt((size_t)nch * nb);
    std::vector<float> Z((size_t)nch * zstride * 2, 0.f), dcol;
    g_keep_dcol = &dcol;
    rc = emu_bank_run(fs, fc, cfg.mode, iq, x_len, 0, S, 1, d, P.data(), Pt.data(), Z.data(), nullptr, sizes);   // (asserts dcol == d itself)
    g_keep_dcol = nullptr;
    if (rc) return -104;
    if (G % 25 == 0 || des.outs_per_slot % 25 != 0) return -105;              // the case wanted: whole tiles per slot, a partial last tile
    // (E_off = 0: every window passes the squelch -- the first slots' noise windows lie in front of a capture this short)
    std::vector<double> Qn((size_t)nch * S, 0.0);
    std::vector<uint64_t> pcol(des.ac.btbb_pcol, des.ac.btbb_pcol + 24);
    const WindowParams p = make_window_params(des, S, nb, 0, 1 << 14, true, pcol.data());
    WindowOut a, b;
    run_window<WinLayout<3, 96, 20>>(des, p, S, nch, d, G, P.data(), Pt.data(), Qn.data(), a);
    // (the rows past the stream's end in the last tile: NaNs, so that a symbol formed from one of them shows)
    for (long long g = G; g < (G + 24) / 25 * 25; g++)
        for (int c = 0; c < 80; c++) dcol[((size_t)(g / 25) * 80 + c) * 25 + g % 25] = __builtin_nanf("");
    run_window<WinLayoutTiled>(des, p, S, nch, dcol.data(), G, P.data(), Pt.data(), Qn.data(), b);
    counts_out[0] = (int)a.counts[0]; counts_out[1] = (int)a.counts[1];
    const size_t W = (size_t)S * nch;
    if (!same_bytes(a.win_len, b.win_len, W)) return -1;
    if (a.counts[0] != b.counts[0]) return -2;
    if (!same_bytes(a.hits, b.hits, std::min<size_t>(a.counts[0], (size_t)p.max_hits))) return -3;
    if (a.counts[1] != b.counts[1]) return -4;
    if (!same_bytes(a.fin, b.fin, a.counts[1])) return -5;
    if (!same_bytes(a.symbits, b.symbits, a.symbits.size())) return -6;
    if (!same_bytes(a.win_fin, b.win_fin, W)) return -7;
    if (!same_bytes(a.winbits, b.winbits, a.winbits.size())) return -8;
    return (int)a.counts[0];
}
