// fd_fxbank.hip -- the effect banks of fd_fxbank.hpp: buffers, configuration, clone and launch of each family (host code; the kernels are in
// fd_fdn.hip, fd_reverb3.hip, fd_fdnx.hip, fd_fbdelay.hip, fd_resynth.hip and fd_convolve.hip; those of the networks' fused mix-down in fd_fxmix.hip).
#include <algorithm>
#include <cmath>
#include <vector>

#include "fd_fxbank.hpp"
#include "fd_convolve.hpp"
#include "fd_fbdelay.hpp"
#include "fd_fdnx.hpp"
#include "fd_opts.hpp"
#include "fd_resynth.hpp"
#include "fd_reverb3.hpp"

namespace fd {
namespace {

int hip_fail(hipError_t e, const std::string& what) {
    return api_fail(e == hipErrorOutOfMemory ? FDSP_ENOMEM : FDSP_EDEVICE, what + ": " + hipGetErrorString(e));
}
int launch_error() { const hipError_t e = hipGetLastError(); return e == hipSuccess ? FDSP_OK : hip_fail(e, "hipGetLastError()"); }

// A family's device buffers as one list of (pointer, bytes): allocated all or none, freed, and copied (a clone, or what outlives a rate
// change) by walking it.  An entry of 0 bytes is a buffer the instance does not have: it stays NULL.
struct Buf { void** p; size_t bytes; };
using Bufs = std::vector<Buf>;

void free_bufs(const Bufs& l) {
    for (const Buf& b : l) {
        if (*b.p) hipFree(*b.p);
        *b.p = nullptr;
    }
}
hipError_t alloc_bufs(const Bufs& l) {
    for (const Buf& b : l) *b.p = nullptr;
    hipError_t e = hipSuccess;
    for (const Buf& b : l)
        if (e == hipSuccess && b.bytes) e = hipMalloc(b.p, b.bytes);
    if (e != hipSuccess) free_bufs(l);
    return e;
}
// entries [first, ..) of `from` into `to` (lists of the same shape) in stream order; entries `from` does not have are skipped
hipError_t copy_bufs(const Bufs& to, const Bufs& from, hipStream_t s, size_t first = 0) {
    hipError_t e = hipSuccess;
    for (size_t i = first; i < to.size() && e == hipSuccess; i++)
        if (*from[i].p) e = hipMemcpyAsync(*to[i].p, *from[i].p, to[i].bytes, hipMemcpyDeviceToDevice, s);
    return e;
}
// the end of a transactional configuration: entries [first, ..) of the old buffers move into the new ones, the stream drains, the old
// buffers go (on the first configuration the old list is all NULL: nothing to carry or free)
void carry_and_free(const Bufs& to, const Bufs& from, size_t first, hipStream_t s) {
    copy_bufs(to, from, s, first);
    hipStreamSynchronize(s);
    free_bufs(from);
}

// ---- the lane-per-frame networks: rate, bus and the planar staging copy of voice-minor launches ------------------------------------------------
class NetFx : public FxBank {
  public:
    ~NetFx() override {
        free_stage();
        if (mixs_) hipFree(mixs_);
    }
    int inputs() const override { return nin_; }
    int outputs() const override { return nout_; }
    FdnBus* bus() override { return &bus_; }
    int set_sample_rate(double sr, hipStream_t s) override {
        if (sr == sr_) return FDSP_OK;  // Delay::set_sample_rate: nothing happens unless the rate changes
        if (hipError_t e = hipStreamSynchronize(s)) return hip_fail(e, "hipStreamSynchronize");
        return configure(sr, s);
    }
    // built the way this instance was (at its creation rate, where it passed validation) and moved to its rate, then every state buffer
    // is copied (the tables configure computed are already equal)
    int clone(hipStream_t s, std::unique_ptr<FxBank>* out) override {
        std::unique_ptr<NetFx> d = fresh();
        int rc = d->create(sr0_, s);
        if (rc == FDSP_OK) rc = d->set_sample_rate(sr_, s);
        if (rc != FDSP_OK) return rc;
        if (hipError_t e = copy_bufs(d->bufs(), bufs(), s, tables_)) return hip_fail(e, std::string("fdsp_bank_clone: ") + what_ + " state");
        d->bus_ = bus_;
        *out = std::move(d);
        return FDSP_OK;
    }
    // Feedback::process is the per-sample tick (feedback.rs:136-146): both modes are the same arithmetic but for the joins (MultiJoin / Join)
    void render(const float* in, float* out, size_t T, size_t fstride, int layout, int tick, bool capturing, hipStream_t s) override {
        // voice-minor buffers of banks with at least a tile of instances go through the planar staging copy (the lane = frame kernels read
        // 256-byte runs of it instead of gathering a line per frame); the staging buffer grows outside captures only, like the partial mixes
        bool staged = layout == FDSP_LAYOUT_VOICE_MINOR && V_ >= 64 && frames_kernel();
        const size_t need = V_ * (size_t)(nin_ + nout_) * T;
        if (staged && need > stage_n_) {
            if (capturing) staged = false;
            else {
                free_stage();  // (hipFree waits for launches that still use the old buffer)
                if (hipMalloc((void**)&stage_, need * sizeof(float)) == hipSuccess) stage_n_ = need;
                else { (void)hipGetLastError(); stage_ = nullptr; staged = false; }   // no room: the kernels' own voice-minor path
            }
        }
        if (staged) {
            float *pin = stage_, *pout = stage_ + V_ * (size_t)nin_ * T;
            fdn_launch_transpose(in, pin, V_, T, nin_, true, s);
            launch(pin, pout, T, T, FDSP_LAYOUT_PLANAR, tick, s);
            fdn_launch_transpose(pout, out, V_, T, nout_, false, s);
        } else {
            launch(in, out, T, fstride, layout, tick, s);
        }
    }
    int create(double sr, hipStream_t s) { sr0_ = sr; return configure(sr, s); }   // the first configuration

    // ---- the fused mix-down: planar render into the mix scratch, chunk by chunk, then the groups' partials (fd_fxmix.hip) ----
    // The scratch holds one chunk: [V][inputs][L] (the planar copy of the chunk's input) | [V][outputs][L].  A chunk is a multiple of 64
    // frames, so the kernels see whole blocks but for the launch's ragged end, as in any split of a launch -- and these banks render
    // chunked == whole.  Every chunk writes its own columns of the full-length partial buffer.
    bool has_mix() const override { return true; }
    bool mix_reserved(size_t T) const override { return mix_need(T) <= mixs_n_; }
    int mix_reserve(size_t T) override {
        const size_t need = mix_need(T);
        if (need <= mixs_n_) return FDSP_OK;
        float* p = nullptr;
        if (hipError_t e = hipMalloc((void**)&p, need * sizeof(float))) return hip_fail(e, std::string("fdsp_bank_mix_reserve: ") + what_ + " mix scratch");
        if (mixs_) hipFree(mixs_);   // (hipFree waits for launches that still use the old buffer)
        mixs_ = p;
        mixs_n_ = need;
        return FDSP_OK;
    }
    void render_mix(const float* in, float* part, size_t T, size_t fstride, int layout, int tick, const float* panw, size_t pstride, hipStream_t s) override {
        const size_t L = mix_chunk(T);
        // a planar launch that fits the scratch with the caller's own row stride: the input is read in place
        if (layout == FDSP_LAYOUT_PLANAR && T <= L && (size_t)nout_ * fstride <= (size_t)(nin_ + nout_) * L) {
            launch(in, mixs_, T, fstride, FDSP_LAYOUT_PLANAR, tick, s);
            fx_launch_mix_groups(mixs_, V_, nout_, fstride, T, part, T, 0, panw, pstride, s);
            return;
        }
        float *pin = mixs_, *pout = mixs_ + V_ * (size_t)nin_ * L;
        for (size_t t0 = 0; t0 < T; t0 += L) {
            const size_t n = T - t0 < L ? T - t0 : L;
            if (layout == FDSP_LAYOUT_VOICE_MINOR) fx_launch_stage_in(in, pin, V_, T, nin_, t0, n, L, s);
            else fx_launch_copy_rows(in + t0, fstride, pin, L, V_ * (size_t)nin_, n, s);   // (one stride per launch: the chunk's rows move over)
            launch(pin, pout, n, L, FDSP_LAYOUT_PLANAR, tick, s);
            fx_launch_mix_groups(pout, V_, nout_, L, n, part, T, t0, panw, pstride, s);
        }
    }

  protected:
    // frames per chunk of a launch of T frames: the option, else what the byte budget holds; never more than the launch in whole blocks
    size_t mix_chunk(size_t T) const {
        size_t L = (size_t)tl_opts.fx_mix_chunk_frames;
        if (L == 0) L = MIX_SCRATCH_BYTES / (V_ * (size_t)(nin_ + nout_) * sizeof(float)) / 64 * 64;
        L = L < 64 ? 64 : (L > MIX_CHUNK_MAX ? MIX_CHUNK_MAX : L);
        const size_t whole = (T + 63) / 64 * 64;
        return whole < L ? whole : L;
    }
    size_t mix_need(size_t T) const { return V_ * (size_t)(nin_ + nout_) * mix_chunk(T); }
    static constexpr size_t MIX_SCRATCH_BYTES = (size_t)256 << 20;   // the automatic chunk's budget: the fastest of 16 / 64 / 256 MiB
    static constexpr size_t MIX_CHUNK_MAX = (size_t)1 << 21;        // frames: the grids of the transpose-in and the partial kernel
    NetFx(size_t V, const char* what) : V_(V), what_(what) {}
    // (re)allocate the lines for a sample rate.  Transactional: the constants are validated and the new buffers allocated BEFORE anything of
    // the instance changes; on any failure it keeps its old constants, buffers and rate
    virtual int configure(double sr, hipStream_t s) = 0;
    virtual std::unique_ptr<NetFx> fresh() const = 0;    // the same network, no buffers yet
    virtual Bufs bufs() = 0;                             // every state buffer of the current configuration
    virtual bool frames_kernel() const { return true; }  // the launch takes a lane = frame kernel (the staging copy pays)
    virtual void launch(const float* in, float* out, size_t T, size_t fstride, int layout, int tick, hipStream_t s) = 0;
    void free_stage() { if (stage_) hipFree(stage_); stage_ = nullptr; stage_n_ = 0; }

    size_t V_, tables_ = 0;         // instances; leading entries of bufs() that configure computes from the description
    double sr0_ = 0.0, sr_ = 0.0;   // the creation rate, the current one
    int nin_ = 2, nout_ = 2;
    FdnBus bus_;
    const char* what_;
    float* stage_ = nullptr;   // planar staging of voice-minor launches: [V][inputs][frames] | [V][outputs][frames] (fd_fdn.hip "voice-minor I/O")
    size_t stage_n_ = 0;
    float* mixs_ = nullptr;    // the mix scratch: apart from stage_, allocated by mix_reserve alone, never shrunk, not cloned
    size_t mixs_n_ = 0;
};

// reverb_stereo, reverb4_stereo and the generic network (fd_fdn.hpp): one kernel family, three ways to make its constants
class HadamardFx final : public NetFx {
  public:
    enum Kind { REVERB, REVERB4, GENERIC };
    HadamardFx(Kind kind, double room, double time, double damping, const FdnDesc& desc, size_t V)
        : NetFx(V, "reverb"), kind_(kind), room_(room), time_(time), damping_(damping), desc_(desc) {}
    ~HadamardFx() override { free_bufs(bufs()); }
    hipError_t reset(hipStream_t s) override { fdn_launch_reset(c_, st_, V_, s); return hipGetLastError(); }

  private:
    int configure(double sr, hipStream_t s) override {
        FdnConst c;
        if (kind_ == GENERIC) fdn_make_const_generic(desc_, sr, &c);
        else if (kind_ == REVERB4) fdn_make_const_reverb4(room_, time_, sr, &c);
        else fdn_make_const(room_, time_, damping_, sr, &c);
        for (int i = 0; i < c.lines; i++)
            if (c.len[i] <= 128)   // len = delay + 1: a delay of 128 samples is the shortest
                return api_fail(FDSP_EINVAL, kind_ == GENERIC ? "fdsp_fdn_create: every delay must be at least 128 samples at the bank's sample rate (two blocks: the lane-per-frame kernel's rule)"
                                                               : "reverb_stereo / reverb4_stereo: every delay must be at least 128 samples (room_size * sample_rate too small)");
        if (kind_ != REVERB && c.cap > (1 << 18))
            return api_fail(FDSP_EINVAL, "reverb4_stereo / fdsp_fdn_create: delays of more than 2^18 samples (too long for the lane-per-frame kernel at this sample rate)");
        FdnState st{};
        if (hipError_t e = alloc_bufs(bufs(c, st))) return hip_fail(e, "reverb_stereo buffers");
        // The new lines start empty (Delay::set_sample_rate resizes and resets, delay.rs:105-113) -- but a change of rate resets nothing else: the
        // FIRs keep their two samples of history (Fir::set_sample_rate, fir.rs:52-54) and Feedback its value (feedback.rs:125-127), so a tail that
        // is sounding when the rate changes goes on from those, exactly like the reference's
        fdn_launch_reset(c, st, V_, s);
        carry_and_free(bufs(c, st), bufs(c_, st_), 2, s);   // v1, v2, fb
        c_ = c; st_ = st; sr_ = sr;
        nin_ = c.nin; nout_ = c.nout;
        return launch_error();
    }
    Bufs bufs(const FdnConst& c, FdnState& st) const {
        const size_t n = V_;
        return {{(void**)&st.rings, n * c.ring_stride * sizeof(float)}, {(void**)&st.wpos, n * sizeof(int)}, {(void**)&st.v1, n * 32 * sizeof(float)},
                {(void**)&st.v2, n * 32 * sizeof(float)}, {(void**)&st.fb, n * 32 * sizeof(float)}};
    }
    Bufs bufs() override { return bufs(c_, st_); }
    std::unique_ptr<NetFx> fresh() const override { return std::make_unique<HadamardFx>(kind_, room_, time_, damping_, desc_, V_); }
    bool frames_kernel() const override { return c_.generic || tl_opts.fdn_kernel == 0 || c_.sections == 2; }
    void launch(const float* in, float* out, size_t T, size_t fstride, int layout, int tick, hipStream_t s) override { fdn_launch_render(c_, st_, V_, in, out, T, fstride, layout, tick, s, bus_); }

    Kind kind_;
    double room_, time_, damping_;
    FdnDesc desc_;
    FdnConst c_{};
    FdnState st_{};
};

// reverb4_stereo_delays(times, time) with one delay table for the bank or one per instance (fd_fdn.hpp "PER INSTANCE"): the host keeps the
// delays in seconds, the device a table of ring lengths at the current rate.  A change of rate re-derives every row, checks the two-block
// rule over all of them and carries the FIR history and the feedback value like the uniform reverbs.
class Reverb4TableFx final : public NetFx {
  public:
    Reverb4TableFx(std::vector<float> delays, int per_instance, double time, double hold_seconds, size_t V)
        : NetFx(V, "reverb4_stereo_delays"), d_(std::move(delays)), per_(per_instance), time_(time), hold_(hold_seconds) { tables_ = 1; }
    ~Reverb4TableFx() override { free_bufs(bufs()); }
    hipError_t reset(hipStream_t s) override { fdn_launch_reset(c_, st_, V_, s); return hipGetLastError(); }
    // every row is valid at the CURRENT rate (the creation's, the last change's or fdsp_reverb4_set_delays' check): the clone is built there
    int clone(hipStream_t s, std::unique_ptr<FxBank>* out) override {
        auto d = std::make_unique<Reverb4TableFx>(d_, per_, time_, hold_, V_);
        if (int rc = d->create(sr_, s)) return rc;
        if (hipError_t e = copy_bufs(d->bufs(), bufs(), s, tables_)) return hip_fail(e, "fdsp_bank_clone: reverb4_stereo_delays state");
        d->bus_ = bus_;
        *out = std::move(d);
        return FDSP_OK;
    }
    // rows first .. first+count-1 (instances, or the single row 0 of a bank with one table), checked before anything changes; then the
    // table rows are uploaded and those instances reset (the whole bank where it shares one row), in stream order
    int set_delays(const float* rows, size_t first, size_t count, hipStream_t s) {
        const size_t nrows = per_ ? V_ : 1;
        if (first > nrows || count > nrows - first)
            return api_fail(FDSP_EINVAL, "fdsp_reverb4_set_delays: rows out of range (one row per instance with per_instance, else the single row 0)");
        std::vector<int> lens(count * 32);
        for (size_t i = 0; i < count * 32; i++) {
            if (!(rows[i] >= 0.0f) || !(rows[i] < 1e6f)) return api_fail(FDSP_EINVAL, "fdsp_reverb4_set_delays: a delay is negative or not a number (Delay::new asserts time >= 0)");
            const double samples = std::round((double)rows[i] * sr_);
            if (samples < 128.0)
                return api_fail(FDSP_EINVAL, "fdsp_reverb4_set_delays: every delay must be at least 128 samples at the bank's sample rate (two blocks: the lane-per-frame kernel's rule)");
            if (samples + 1.0 > (double)c_.cap)
                return api_fail(FDSP_EINVAL, "fdsp_reverb4_set_delays: a delay of " + std::to_string((long long)samples) + " samples needs a larger ring than the bank's " +
                                                 std::to_string(c_.cap) + " slots (sized at creation from the longest delay given, at least 0.105 s)");
            lens[i] = (int)samples + 1;
        }
        if (count == 0) return FDSP_OK;
        std::copy(rows, rows + count * 32, d_.begin() + first * 32);
        hipError_t e = hipMemcpyAsync(tab_ + first * 32, lens.data(), lens.size() * sizeof(int), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) {
            const size_t i0 = per_ ? first : 0, n = per_ ? count : V_;
            FdnState part = st_;
            part.rings += i0 * c_.ring_stride; part.wpos += i0; part.v1 += i0 * 32; part.v2 += i0 * 32; part.fb += i0 * 32;
            fdn_launch_reset(c_, part, n, s);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(s);   // (lens is a local, rows is borrowed)
        return e == hipSuccess ? FDSP_OK : hip_fail(e, "fdsp_reverb4_set_delays");
    }

  private:
    int configure(double sr, hipStream_t s) override {
        const size_t rows = per_ ? V_ : 1;
        std::vector<int> lens(rows * 32);
        FdnConst c;
        const int shortest = fdn_make_table_reverb4(d_.data(), rows, time_, sr, hold_, lens.data(), &c);
        if (shortest < 0) return api_fail(FDSP_EINVAL, "fdsp_reverb4_stereo_delays_create: delays of more than 2^18 samples (too long for the lane-per-frame kernel at this sample rate)");
        if (shortest < 128)
            return api_fail(FDSP_EINVAL, "fdsp_reverb4_stereo_delays_create: every delay must be at least 128 samples at the bank's sample rate (two blocks: the lane-per-frame kernel's rule)");
        FdnState st{};
        int* tab = nullptr;
        hipError_t e = alloc_bufs(bufs(c, st, tab));
        if (e == hipSuccess && (e = hipMemcpyAsync(tab, lens.data(), lens.size() * sizeof(int), hipMemcpyHostToDevice, s)) != hipSuccess) free_bufs(bufs(c, st, tab));
        if (e != hipSuccess) return hip_fail(e, "fdsp_reverb4_stereo_delays_create buffers");
        fdn_launch_reset(c, st, V_, s);   // new lines start empty; the FIRs' history and the feedback value stay (HadamardFx::configure)
        carry_and_free(bufs(c, st, tab), bufs(c_, st_, tab_), 3, s);   // v1, v2, fb (and the stream drains before `lens` goes)
        c_ = c; st_ = st; tab_ = tab; sr_ = sr;
        return launch_error();
    }
    Bufs bufs(const FdnConst& c, FdnState& st, int*& tab) const {
        const size_t n = V_;
        return {{(void**)&tab, (per_ ? n : 1) * 32 * sizeof(int)}, {(void**)&st.rings, n * c.ring_stride * sizeof(float)}, {(void**)&st.wpos, n * sizeof(int)},
                {(void**)&st.v1, n * 32 * sizeof(float)}, {(void**)&st.v2, n * 32 * sizeof(float)}, {(void**)&st.fb, n * 32 * sizeof(float)}};
    }
    Bufs bufs() override { return bufs(c_, st_, tab_); }
    std::unique_ptr<NetFx> fresh() const override { return std::make_unique<Reverb4TableFx>(d_, per_, time_, hold_, V_); }
    void launch(const float* in, float* out, size_t T, size_t fstride, int layout, int tick, hipStream_t s) override {
        fdn_launch_render_reverb4_table(c_, st_, tab_, per_ ? 32 : 0, V_, in, out, T, fstride, layout, tick, s, bus_);
    }

    std::vector<float> d_;   // [rows][32] seconds, as given (f32: Delay::new(d as f64))
    int per_;
    double time_, hold_;     // hold_: the delay the rings hold at least, fixed at creation
    FdnConst c_{};
    FdnState st_{};
    int* tab_ = nullptr;     // [rows][32] ring lengths at sr_
};

// reverb3_stereo (fd_reverb3.hpp): what the reference's Reverb::set_sample_rate leaves alone survives a new rate (the `pre` diffusers
// entirely; every allpass's z, the feedback sample and the filters' values: rv3_launch_migrate); the first configuration zeroes everything
class Reverb3Fx final : public NetFx {
  public:
    Reverb3Fx(double time, double diffusion, const Rv3Filter& flt, size_t V) : NetFx(V, "reverb3"), time_(time), diffusion_(diffusion), flt_(flt) {}
    ~Reverb3Fx() override { free_bufs(bufs()); }
    hipError_t reset(hipStream_t s) override { rv3_launch_reset(c_, st_, V_, s); return hipGetLastError(); }

  private:
    int configure(double sr, hipStream_t s) override {
        Rv3Const c;
        if (!rv3_make_const(time_, diffusion_, flt_, sr, &c))
            // rv3_make_const: the shortest line, round(400 / 44100 * sr) + 1, reaches 129 at 14056.875 Hz; the longest, round(1123 / 44100 * sr) + 1, passes 2^20 at 41.177 MHz
            return api_fail(FDSP_EINVAL, "reverb3_stereo: every delay must exceed 128 samples at the bank's sample rate (two blocks: the lane-per-frame kernel's rule; >= 14057 Hz) "
                                         "and none may exceed 2^20 samples (< 41.17 MHz)");
        const bool first = st_.pre == nullptr;
        Rv3State st = st_;   // (pre, wpre and fval are allocated once)
        if (hipError_t e = alloc_bufs(bufs(c, st, first))) return hip_fail(e, "reverb3_stereo buffers");
        if (first) rv3_launch_init(c, st, V_, s);
        else {
            // the new lines start empty; pre / filter values stay where they are; z and the feedback sample move over
            hipMemsetAsync(st.rings, 0, V_ * c.ring_stride * sizeof(float), s);
            hipMemsetAsync(st.wpos, 0, V_ * sizeof(int), s);
            rv3_launch_migrate(c_, st_, c, st, V_, s);
        }
        carry_and_free(bufs(c, st, false), bufs(c_, st_, false), 2, s);   // (the old lines go, nothing to carry)
        c_ = c; st_ = st; sr_ = sr;
        return launch_error();
    }
    // the lines of a rate (rings, write positions), with `all` also what outlives a rate change
    Bufs bufs(const Rv3Const& c, Rv3State& st, bool all) const {
        const size_t n = V_;
        Bufs l = {{(void**)&st.rings, n * c.ring_stride * sizeof(float)}, {(void**)&st.wpos, n * sizeof(int)}};
        if (all) l.insert(l.end(), {{(void**)&st.pre, n * 4 * (RV3_PRE_CAP + 64) * sizeof(float)}, {(void**)&st.wpre, n * sizeof(int)}, {(void**)&st.fval, n * 32 * sizeof(float)}});
        return l;
    }
    Bufs bufs() override { return bufs(c_, st_, true); }
    std::unique_ptr<NetFx> fresh() const override { return std::make_unique<Reverb3Fx>(time_, diffusion_, flt_, V_); }
    void launch(const float* in, float* out, size_t T, size_t fstride, int layout, int, hipStream_t s) override {
        rv3_launch_render(c_, st_, V_, in, out, T, fstride, layout, s, bus_);   // (Reverb has no process override: one arithmetic)
    }

    double time_, diffusion_;
    Rv3Filter flt_;
    Rv3Const c_{};
    Rv3State st_{};
};

// The line networks -- filtered / per-instance Hadamard networks (fd_fdnx.hpp) and feedback delay banks (fd_fbdelay.hpp): one life cycle
// around one description (FdnxDesc).  What a family supplies: its table row and constants, how to make them, when a table is refused and
// in which words, its inputs and outputs, and its launch.
struct FdnxFamily {
    using Row = FdnxInst;
    using Const = FdnxConst;
    static constexpr const char* what = "network";
    static constexpr const char* who = "fdsp_fdn_network_create";
    static constexpr const char* too_long = ": delays of more than 2^18 samples (too long for the lane-per-frame kernel at this sample rate)";
    static int make_table(const FdnxDesc& d, size_t V, double sr, std::vector<Row>& tab, Const* c) { return fdnx_make_table(d, V, sr, tab, c); }
    static bool refused(int shortest, const Const&) { return shortest < 0; }
    static int nin(const Const& c) { return c.nin; }
    static int nout(const Const& c) { return c.nout; }
    static void launch(const Const& c, const FdnxState& st, size_t V, const float* in, float* out, size_t T, size_t fstride, int layout, int tick,
                       hipStream_t s, const FdnBus& bus) {
        fdnx_launch_render(c, st, V, in, out, T, fstride, layout, tick, s, bus);
    }
};
struct FbFamily {
    using Row = FbInst;
    using Const = FbConst;
    static constexpr const char* what = "feedback_delay";
    static constexpr const char* who = "fdsp_feedback_delay_create";
    static constexpr const char* too_long = ": no ring may exceed 2^18 slots (a delay too long for the lane-per-frame kernel at this sample rate)";
    static int make_table(const FdnxDesc& d, size_t V, double sr, std::vector<Row>& tab, Const* c) { return fb_make_table(d, V, sr, tab, c); }
    static bool refused(int shortest, const Const& c) { return shortest < 0 || c.cap > (1 << 18); }
    static int nin(const Const& c) { return c.lines; }
    static int nout(const Const& c) { return c.lines; }
    // Feedback::process is the per-sample tick and these graphs have no join: one arithmetic for both modes
    static void launch(const Const& c, const FdnxState& st, size_t V, const float* in, float* out, size_t T, size_t fstride, int layout, int,
                       hipStream_t s, const FdnBus& bus) {
        fb_launch_render(c, st, V, in, out, T, fstride, layout, s, bus);
    }
};

// the table and the lines for a sample rate.  The new rings start empty (Delay::set_sample_rate, delay.rs:105-113), the coefficients follow
// the rate (filter.rs:58-61, svf.rs:989-992), and the Fir carry, the filter states and the feedback value stay (fir.rs:52-54,
// feedback.rs:125-127, 254-257)
template <class F>
class LineFx final : public NetFx {
    using Row = typename F::Row;
    using Const = typename F::Const;

  public:
    LineFx(const FdnxDesc& d, size_t V) : NetFx(V, F::what), d_(d) { tables_ = 1; }
    ~LineFx() override { free_bufs(bufs()); }
    hipError_t reset(hipStream_t s) override { fdnx_launch_reset(c_.ring_stride, st_, V_, s); return hipGetLastError(); }

  private:
    int configure(double sr, hipStream_t s) override {
        const std::string who = F::who;
        std::vector<Row> tab;
        Const c;
        const int shortest = F::make_table(d_, V_, sr, tab, &c);
        if (F::refused(shortest, c)) return api_fail(FDSP_EINVAL, who + F::too_long);
        if (shortest < 128)
            return api_fail(FDSP_EINVAL, who + ": every delay must be at least 128 samples at the bank's sample rate (two blocks: the lane-per-frame kernel's rule)");
        FdnxState st{};
        hipError_t e = alloc_bufs(bufs(c, st));
        if (e == hipSuccess && (e = hipMemcpyAsync((void*)c.tab, tab.data(), tab.size() * sizeof(Row), hipMemcpyHostToDevice, s)) != hipSuccess) free_bufs(bufs(c, st));
        if (e != hipSuccess) return hip_fail(e, who + " buffers");
        fdnx_launch_reset(c.ring_stride, st, V_, s);
        carry_and_free(bufs(c, st), bufs(c_, st_), 3, s);   // v1, v2, fb, s1, s2 (and the stream drains before `tab` goes)
        c_ = c; st_ = st; sr_ = sr;
        nin_ = F::nin(c); nout_ = F::nout(c);
        return launch_error();
    }
    Bufs bufs(Const& c, FdnxState& st) const {
        const size_t n = V_;
        return {{(void**)&c.tab, (c.tab_stride ? n : 1) * sizeof(Row)}, {(void**)&st.rings, n * c.ring_stride * sizeof(float)},
                {(void**)&st.wpos, n * sizeof(int)}, {(void**)&st.v1, n * 32 * sizeof(float)}, {(void**)&st.v2, n * 32 * sizeof(float)},
                {(void**)&st.fb, n * 32 * sizeof(float)}, {(void**)&st.s1, n * 32 * sizeof(float)}, {(void**)&st.s2, n * 32 * sizeof(float)}};
    }
    Bufs bufs() override { return bufs(c_, st_); }
    std::unique_ptr<NetFx> fresh() const override { return std::make_unique<LineFx>(d_, V_); }
    void launch(const float* in, float* out, size_t T, size_t fstride, int layout, int tick, hipStream_t s) override { F::launch(c_, st_, V_, in, out, T, fstride, layout, tick, s, bus_); }

    FdnxDesc d_;
    Const c_{};
    FdnxState st_{};
};

int make_net(std::unique_ptr<NetFx> f, double sr, hipStream_t s, std::unique_ptr<FxBank>* out) {
    if (int rc = f->create(sr, s)) return rc;
    *out = std::move(f);
    return FDSP_OK;
}

// ---- resynthesizer banks (fd_resynth.hpp): tables, frame ring, input ring, device sample counter -------------------------------------------
class ResynthFx final : public FxBank {
  public:
    // (the table pointers of `c` are another instance's)
    ResynthFx(const RsConst& c, int ftz, size_t V, const RsFn& fn = RsFn{}, std::shared_ptr<const std::vector<char>> code = nullptr)
        : c_(c), fn_(fn), code_(std::move(code)), ftz_(ftz), V_(V) {
        for (const Buf& b : bufs()) *b.p = nullptr;
        fn_.process = nullptr;
    }
    ~ResynthFx() override {
        free_bufs(bufs());
        if (mod_) hipModuleUnload(mod_);
    }
    int inputs() const override { return c_.I; }
    int outputs() const override { return c_.O; }
    // FftWindow::set_sample_rate: frequency() follows, every other state stays (resynth.rs:170-172, 325-330).  The bin spacing lives in device
    // memory, in stream order behind the last render: a captured launch replays with the new rate
    int set_sample_rate(double sr, hipStream_t s) override {
        const float fstep = (float)sr / (float)c_.N;
        const float srf = (float)sr;   // FftWindow::set_sample_rate(sample_rate as f32): what a closure's time() family divides by
        hipError_t e = hipMemcpyAsync(st_.fstep, &fstep, sizeof(float), hipMemcpyHostToDevice, s);
        if (e == hipSuccess && fn_.srf) e = hipMemcpyAsync(fn_.srf, &srf, sizeof(float), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);   // (fstep and srf are locals)
        return e == hipSuccess ? FDSP_OK : hip_fail(e, "fdsp_bank_set_sample_rate");
    }
    // Resynth::reset: the sample count and the four windows start over (resynth.rs:332-337)
    // ... and a closure's state starts over with them (a fresh closure)
    hipError_t reset(hipStream_t s) override {
        hipError_t e = hipMemsetAsync(st_.samples, 0, sizeof(unsigned long long), s);
        if (e == hipSuccess && fn_.state) e = hipMemsetAsync(fn_.state, 0, state_bytes(), s);
        return e;
    }
    // a new bank with zero band / gain tables, then everything but the window and twiddle tables copied over (a closure's parameters and
    // state among it; its module is loaded from the same code object)
    int clone(hipStream_t s, std::unique_ptr<FxBank>* out) override {
        auto d = std::make_unique<ResynthFx>(c_, ftz_, V_, fn_, code_);
        const Bufs l = bufs();
        const std::vector<float> band(l[7].bytes / sizeof(float)), gain(l[8].bytes / sizeof(float));
        if (int rc = d->init(band.data(), gain.data(), s)) return rc;
        if (hipError_t e = copy_bufs(d->bufs(), l, s, 3)) return hip_fail(e, "fdsp_bank_clone: resynthesizer state");
        *out = std::move(d);
        return FDSP_OK;
    }
    // Resynth has no process override: FDSP_MODE_PROCESS == FDSP_MODE_TICK
    void render(const float* in, float* out, size_t T, size_t fstride, int layout, int, bool, hipStream_t s) override {
        if (c_.proc == RS_FN) (ftz_ ? rs_ftz::rs_launch_render_fn : rs_ieee::rs_launch_render_fn)(c_, st_, fn_, V_, in, out, T, fstride, layout, s);
        else (ftz_ ? rs_ftz::rs_launch_render : rs_ieee::rs_launch_render)(c_, st_, V_, in, out, T, fstride, layout, s);
    }
    // the buffers, the tables uploaded (band [rows][O][2] and gain [rows][O][N/2 + 1] where the processor has them), empty windows at 44.1 kHz
    int init(const float* band, const float* gain, hipStream_t s) {
        const Bufs l = bufs();
        const float fstep = (float)FDSP_DEFAULT_SR / (float)c_.N, srf = (float)FDSP_DEFAULT_SR;
        std::vector<float> tw(c_.N), hann(c_.N), hz(c_.N);
        rs_tables(c_.N, hann.data(), hz.data(), tw.data());
        if (code_) {   // a closure bank: its module on this device, before anything is allocated
            if (hipModuleLoadData(&mod_, code_->data()) != hipSuccess) { mod_ = nullptr; (void)hipGetLastError(); return api_fail(FDSP_EDEVICE, "fdsp_resynth_fn_create: hipModuleLoadData failed for the compiled functor"); }
            if (hipModuleGetFunction(&fn_.process, mod_, "rs_process") != hipSuccess) { (void)hipGetLastError(); return api_fail(FDSP_EDEVICE, "fdsp_resynth_fn_create: the compiled functor lacks its entry point"); }
        }
        hipError_t e = alloc_bufs(l);
        if (e == hipSuccess) e = hipMemcpyAsync((void*)c_.tw, tw.data(), l[0].bytes, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync((void*)c_.hann, hann.data(), l[1].bytes, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync((void*)c_.hz, hz.data(), l[2].bytes, hipMemcpyHostToDevice, s);
        if (e == hipSuccess && c_.band) e = hipMemcpyAsync((void*)c_.band, band, l[7].bytes, hipMemcpyHostToDevice, s);
        if (e == hipSuccess && c_.gain) e = hipMemcpyAsync((void*)c_.gain, gain, l[8].bytes, hipMemcpyHostToDevice, s);
        // reset: the windows start empty (nothing is read before a frame of this run exists, but the rings start defined)
        if (e == hipSuccess) e = hipMemsetAsync(st_.samples, 0, sizeof(unsigned long long), s);
        if (e == hipSuccess) e = hipMemcpyAsync(st_.fstep, &fstep, sizeof(float), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemsetAsync(st_.frames, 0, l[3].bytes, s);
        if (e == hipSuccess) e = hipMemsetAsync(st_.xin, 0, l[4].bytes, s);
        for (size_t i = 9; i < l.size() && e == hipSuccess; i++)   // a closure bank's workspace, parameters, state: defined from the start
            if (l[i].bytes) e = hipMemsetAsync(*l[i].p, 0, l[i].bytes, s);
        if (e == hipSuccess && fn_.srf) e = hipMemcpyAsync(fn_.srf, &srf, sizeof(float), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        return e == hipSuccess ? FDSP_OK : hip_fail(e, "fdsp_resynth_create buffers");
    }
    size_t state_bytes() const { return V_ * (size_t)(c_.N / 2 + 1) * fn_.S * sizeof(float); }
    Bufs bufs() {   // the constant tables first
        const size_t N = (size_t)c_.N, rows = (size_t)c_.rows * c_.O;
        const bool fn = c_.proc == RS_FN;
        return {{(void**)&c_.tw, N / 2 * sizeof(float2)}, {(void**)&c_.hann, N * sizeof(float)}, {(void**)&c_.hz, N * sizeof(float)},
                {(void**)&st_.frames, (size_t)c_.R * V_ * c_.O * N * sizeof(float)}, {(void**)&st_.xin, V_ * (size_t)c_.I * c_.Rx * sizeof(float)},
                {(void**)&st_.samples, sizeof(unsigned long long)}, {(void**)&st_.fstep, sizeof(float)},
                {(void**)&c_.band, c_.proc == RS_BAND ? rows * sizeof(float2) : 0}, {(void**)&c_.gain, c_.proc == RS_GAIN ? rows * (N / 2 + 1) * sizeof(float) : 0},
                // a closure bank's part (0 bytes on a stock bank: the pointers stay NULL)
                {(void**)&fn_.x, fn ? V_ * fn_.Fc * (size_t)c_.I * (N / 2 + 1) * sizeof(float2) : 0}, {(void**)&fn_.y, fn ? V_ * fn_.Fc * (size_t)c_.O * (N / 2 + 1) * sizeof(float2) : 0},
                {(void**)&fn_.params, fn ? V_ * (size_t)fn_.P * sizeof(float) : 0}, {(void**)&fn_.state, fn ? state_bytes() : 0}, {(void**)&fn_.srf, fn ? sizeof(float) : 0}};
    }

    RsConst c_;
    RsFn fn_;
    std::shared_ptr<const std::vector<char>> code_;   // the process module's code object (shared by the banks of one functor)
    hipModule_t mod_ = nullptr;
    RsState st_{};
    int ftz_;   // 1: the flush-to-zero instantiation (a Feedback node in front)
    size_t V_;
};

// ---- convolver banks (fd_convolve.hpp): twiddles, taps, response spectra, input / spectrum / pending rings, device counter and lengths ------
class ConvolveFx final : public FxBank {
  public:
    // (the pointers of `c` are another instance's)
    ConvolveFx(const CvConst& c, int ftz, size_t V, size_t max_len) : c_(c), ftz_(ftz), V_(V), max_len_(max_len) { for (const Buf& b : bufs()) *b.p = nullptr; }
    ~ConvolveFx() override { free_bufs(bufs()); }
    int inputs() const override { return c_.I; }   // (a plain bank has I = C; a routed one shares an input among several outputs)
    int outputs() const override { return c_.C; }
    // Convolver has no set_sample_rate override: the response's own rate is ignored and nothing depends on the bank's
    int set_sample_rate(double, hipStream_t) override { return FDSP_OK; }
    // Convolver::reset: the history goes; no block before the new sample 0 is read again
    hipError_t reset(hipStream_t s) override { return hipMemsetAsync(st_.samples, 0, sizeof(unsigned long long), s); }
    int clone(hipStream_t s, std::unique_ptr<FxBank>* out) override {
        auto d = std::make_unique<ConvolveFx>(c_, ftz_, V_, max_len_);
        d->M_ = M_;
        hipError_t e = alloc_bufs(d->bufs());
        if (e == hipSuccess) e = copy_bufs(d->bufs(), bufs(), s);
        if (e != hipSuccess) return hip_fail(e, "fdsp_bank_clone: convolver buffers");
        *out = std::move(d);
        return FDSP_OK;
    }
    // every split of an input into launches gives the same bits: FDSP_MODE_PROCESS == FDSP_MODE_TICK
    void render(const float* in, float* out, size_t T, size_t fstride, int layout, int, bool, hipStream_t s) override {
        (ftz_ ? cv_ftz::cv_launch_render : cv_ieee::cv_launch_render)(c_, st_, V_, in, out, T, fstride, layout, s);
    }
    // the buffers, the twiddles, the rings defined, then the response [rows][NT][len] (NT = C but in a summing bank)
    int init(const float* response, size_t len, hipStream_t s) {
        const Bufs l = bufs();
        std::vector<float> tw(2 * (size_t)c_.B);
        rs_tables(2 * c_.B, nullptr, nullptr, tw.data());
        hipError_t e = alloc_bufs(l);
        if (e == hipSuccess) e = hipMemcpyAsync((void*)c_.tw, tw.data(), l[0].bytes, hipMemcpyHostToDevice, s);
        for (size_t i = 3; i < l.size() && e == hipSuccess; i++) e = hipMemsetAsync(*l[i].p, 0, l[i].bytes, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);   // (tw is a local)
        if (e != hipSuccess) return hip_fail(e, "fdsp_convolve_create buffers");
        if (int rc = set_response(response, len, 0, (size_t)c_.rows, s)) return rc;
        e = hipStreamSynchronize(s);
        return e == hipSuccess ? FDSP_OK : hip_fail(e, "fdsp_convolve_create response");
    }
    int check_response(size_t len, size_t first, size_t count) const {
        const size_t rows = (size_t)c_.rows;
        if (len < 1 || len > max_len_)
            return api_fail(FDSP_EINVAL, "fdsp_convolve_set_response: len = " + std::to_string(len) + " takes 1 .. the bank's max_len = " + std::to_string(max_len_));
        if (first > rows || count > rows - first)
            return api_fail(FDSP_EINVAL, "fdsp_convolve_set_response: rows out of range (one row per instance with per_instance, else the single row 0)");
        if (count != 0 && count != rows && len != M_)
            return api_fail(FDSP_EINVAL, "fdsp_convolve_set_response: a bank has one response length; replacing some of the rows takes the current len = " + std::to_string(M_));
        return FDSP_OK;
    }
    // what re-initialising the node does: new taps (zero beyond len), their partitions' spectra, the lengths, and the history cleared
    int set_response(const float* h, size_t len, size_t first, size_t count, hipStream_t s) {
        const size_t rowf = (size_t)c_.NT * c_.Hcap;
        float* dst = (float*)c_.h + first * rowf;
        const int dims[2] = {(int)len, (int)((len + c_.B - 1) / c_.B)};
        hipError_t e = hipMemsetAsync(dst, 0, count * rowf * sizeof(float), s);
        if (e == hipSuccess) e = hipMemcpy2DAsync(dst, c_.Hcap * sizeof(float), h, len * sizeof(float), len * sizeof(float), count * c_.NT, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(st_.dims, dims, sizeof(dims), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) {
            (ftz_ ? cv_ftz::cv_launch_response : cv_ieee::cv_launch_response)(c_, first, count, s);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = reset(s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);   // (dims is a local, h is borrowed)
        if (e != hipSuccess) return hip_fail(e, "fdsp_convolve_set_response");
        M_ = len;
        return FDSP_OK;
    }
    Bufs bufs() {   // the tables first
        // the input ring and the spectrum ring per (instance, input), the response tables per (row, response row), the rest per (instance, output)
        const size_t B = (size_t)c_.B, B1 = B + 1, rc = (size_t)c_.rows * c_.NT, vc = V_ * c_.C, vi = V_ * c_.I;
        return {{(void**)&c_.tw, B * sizeof(float2)}, {(void**)&c_.h, rc * c_.Hcap * sizeof(float)}, {(void**)&c_.G, rc * c_.Pcap * B1 * sizeof(float2)},
                {(void**)&st_.xin, vi * (size_t)c_.Rx * sizeof(float)}, {(void**)&st_.spec, vi * (size_t)c_.R * B1 * sizeof(float2)},
                {(void**)&st_.zbuf, vc * (size_t)c_.KB * B1 * sizeof(float2)}, {(void**)&st_.pend, vc * (size_t)(c_.KB + 1) * B * sizeof(float)},
                {(void**)&st_.samples, sizeof(unsigned long long)}, {(void**)&st_.dims, 2 * sizeof(int)}};
    }

    CvConst c_;
    CvState st_{};
    int ftz_;   // 1: the flush-to-zero instantiation (a Feedback node in front)
    size_t V_, max_len_, M_ = 0;
};

}  // namespace

int fx_reverb_stereo(size_t instances, int sections, double room_size, double time, double damping, hipStream_t s, std::unique_ptr<FxBank>* out) {
    const HadamardFx::Kind kind = sections == 2 ? HadamardFx::REVERB4 : HadamardFx::REVERB;
    return make_net(std::make_unique<HadamardFx>(kind, room_size, time, damping, FdnDesc(), instances), FDSP_DEFAULT_SR, s, out);
}
int fx_reverb4_delays(size_t instances, const float* delays, int per_instance, double time, hipStream_t s, std::unique_ptr<FxBank>* out) {
    std::vector<float> d(delays, delays + (per_instance ? instances : 1) * 32);
    double hold = FDN_R4_SEARCH_MAX;   // the rings hold the longest delay given or 0.070 s x 1.5, whichever is larger
    for (float x : d) hold = (double)x > hold ? (double)x : hold;
    return make_net(std::make_unique<Reverb4TableFx>(std::move(d), per_instance, time, hold, instances), FDSP_DEFAULT_SR, s, out);
}
int fx_reverb4_set_delays(FxBank* fx, const float* rows, size_t first, size_t count, hipStream_t s) {
    auto* r = dynamic_cast<Reverb4TableFx*>(fx);
    if (!r) return api_fail(FDSP_EINVAL, "fdsp_reverb4_set_delays: not a bank of fdsp_reverb4_stereo_delays_create");
    return r->set_delays(rows, first, count, s);
}
int fx_fdn(size_t instances, int lines, const double* delays, int taps, const float* weights, int inputs, int outputs, hipStream_t s,
           std::unique_ptr<FxBank>* out) {
    FdnDesc d{lines, taps, inputs, outputs};
    for (int i = 0; i < lines; i++) d.delay[i] = delays[i];
    for (int j = 0; j < taps; j++) d.w[j] = weights[j];
    return make_net(std::make_unique<HadamardFx>(HadamardFx::GENERIC, 1.0, 1.0, 0.0, d, instances), FDSP_DEFAULT_SR, s, out);
}
int fx_reverb3_stereo(size_t instances, double time, double diffusion, int svf_mode, float cutoff, float q, float gain, hipStream_t s,
                      std::unique_ptr<FxBank>* out) {
    const Rv3Filter f{svf_mode < 0 ? 0 : 1, svf_mode < 0 ? 0 : svf_mode, cutoff, q, gain};
    return make_net(std::make_unique<Reverb3Fx>(time, diffusion, f, instances), FDSP_DEFAULT_SR, s, out);
}
// the [P][lines] arrays of a C description (fdsp_fdn_network, fdsp_feedback_delay: the same fields) into `d`, whose lines are set
template <class Net>
static void line_desc(FdnxDesc& d, const Net& net, size_t instances) {
    d.taps = net.taps; d.filter = net.filter; d.svf_mode = net.svf_mode; d.place = net.place;
    d.per_instance = net.per_instance ? 1 : 0; d.has_gain = net.line_gain ? 1 : 0;
    const size_t M = (d.per_instance ? instances : 1) * (size_t)d.lines;
    d.delay.assign(net.delays, net.delays + M);
    if (net.taps > 0) d.w.assign(net.weights, net.weights + M * net.taps);
    if (net.filter != FDSP_FDN_FILTER_NONE) d.cutoff.assign(net.cutoff, net.cutoff + M);
    if (net.filter == FDSP_FDN_FILTER_SVF) d.q.assign(net.q, net.q + M);
    if (net.filter == FDSP_FDN_FILTER_SVF && net.svf_mode >= FDSP_SVF_BELL) d.gain.assign(net.gain, net.gain + M);
    if (d.has_gain) d.line_gain.assign(net.line_gain, net.line_gain + M);
}
int fx_fdn_network(size_t instances, const fdsp_fdn_network& net, double sample_rate, hipStream_t s, std::unique_ptr<FxBank>* out) {
    FdnxDesc d;
    d.lines = net.lines; d.nin = net.inputs; d.nout = net.outputs;
    line_desc(d, net, instances);
    return make_net(std::make_unique<LineFx<FdnxFamily>>(d, instances), sample_rate, s, out);
}
int fx_feedback_delay(size_t instances, const fdsp_feedback_delay& net, double sample_rate, hipStream_t s, std::unique_ptr<FxBank>* out) {
    FdnxDesc d;
    d.lines = net.channels; d.has_outer = net.outer_gain ? 1 : 0; d.reverse = net.reverse ? 1 : 0;
    line_desc(d, net, instances);
    if (d.has_outer) d.outer.assign(net.outer_gain, net.outer_gain + (d.per_instance ? instances : 1));
    return make_net(std::make_unique<LineFx<FbFamily>>(d, instances), sample_rate, s, out);
}

// the frame ring of a bank: at least 8 slots, at most a 64 Ki-sample chunk, within 256 MiB where the bank is large
static void rs_ring(RsConst& c, size_t V) {
    const int H = c.N / 4;
    size_t R = ((size_t)256 << 20) / (V * (size_t)c.O * c.N * sizeof(float));
    const size_t rmax = 5 + 65536 / (size_t)H;
    R = R < 8 ? 8 : (R > rmax ? rmax : R);
    c.R = (int)R;
    c.Lmax = (c.R - 5) * H;
}

int fx_resynth(size_t instances, const fdsp_resynth_spec& sp, hipStream_t s, std::unique_ptr<FxBank>* out) {
    const int N = sp.window_length, O = sp.outputs;
    const size_t V = instances;
    RsConst c{};
    c.N = N;
    while ((1 << c.logN) < N) c.logN++;
    c.I = sp.inputs;
    c.O = O;
    c.proc = sp.processor;
    for (int o = 0; o < RS_MAX_CH; o++) c.src[o] = o < O ? sp.source[o] : -1;
    c.rows = sp.per_instance ? (int)V : 1;
    c.invN = 1.0f / (float)N;
    rs_ring(c, V);
    c.Rx = 1;
    while (c.Rx < c.Lmax + N) c.Rx <<= 1;
    std::vector<float> band;
    if (c.proc == FDSP_RESYNTH_BAND)
        for (size_t i = 0; i < (size_t)c.rows * O; i++) band.insert(band.end(), {sp.lo_hz[i], sp.hi_hz[i]});
    auto r = std::make_unique<ResynthFx>(c, sp.flush_denormals, V);
    if (int rc = r->init(band.data(), sp.gain, s)) return rc;
    *out = std::move(r);
    return FDSP_OK;
}

int fx_resynth_fn_compile(const fdsp_resynth_fn_spec& sp, std::shared_ptr<const std::vector<char>>* code) {
    std::string log;
    if (jit_compile_resynth_fn(sp.functor, sp.source, sp.params, sp.state, sp.flush_denormals != 0, code, &log) != 0)
        return api_fail(FDSP_EINVAL, "fdsp_resynth_fn: " + log);
    return FDSP_OK;
}

int fx_resynth_fn(size_t instances, const fdsp_resynth_fn_spec& sp, hipStream_t s, std::unique_ptr<FxBank>* out) {
    std::shared_ptr<const std::vector<char>> code;
    if (int rc = fx_resynth_fn_compile(sp, &code)) return rc;   // before anything is allocated
    const int N = sp.window_length, H = N / 4, I = sp.inputs, O = sp.outputs;
    const size_t V = instances;
    RsConst c{};
    c.N = N;
    while ((1 << c.logN) < N) c.logN++;
    c.I = I;
    c.O = O;
    c.proc = RS_FN;
    for (int o = 0; o < RS_MAX_CH; o++) c.src[o] = -1;
    c.rows = 1;
    c.invN = 1.0f / (float)N;
    rs_ring(c, V);
    // frames per chunk (fd_resynth_fn.hpp): the spectrum workspace within the frame ring's size, at least two frames
    RsFn fn{};
    fn.P = sp.params;
    fn.S = sp.state;
    long long Fc = ((long long)c.R * O * N) / (2LL * (I + O) * (N / 2 + 1));
    Fc = Fc < 2 ? 2 : (Fc > c.R - 4 ? c.R - 4 : Fc);
    fn.Fc = (int)Fc;
    c.Lmax = (fn.Fc - 1) * H;
    c.Rx = 1;
    while (c.Rx < c.Lmax + N) c.Rx <<= 1;
    auto r = std::make_unique<ResynthFx>(c, sp.flush_denormals, V, fn, code);
    if (int rc = r->init(nullptr, nullptr, s)) return rc;
    if (sp.param_values && sp.params > 0) {
        hipError_t e = hipMemcpyAsync(r->fn_.params, sp.param_values, V * (size_t)sp.params * sizeof(float), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);   // (the host array is borrowed)
        if (e != hipSuccess) return hip_fail(e, "fdsp_resynth_fn_create parameters");
    }
    *out = std::move(r);
    return FDSP_OK;
}

int fx_resynth_params(FxBank* fx, size_t first, size_t count, float** row0, size_t* row_floats) {
    auto* r = dynamic_cast<ResynthFx*>(fx);
    if (!r) return api_fail(FDSP_EINVAL, "fdsp_resynth_set_params: not a resynthesizer bank");
    if (r->c_.proc != RS_FN) return api_fail(FDSP_ENOTSUP, "fdsp_resynth_set_params: a stock-processor bank has no closure parameters (fdsp_resynth_set_band / _gain)");
    if (first > r->V_ || count > r->V_ - first) return api_fail(FDSP_EINVAL, "fdsp_resynth_set_params: instances out of range");
    *row_floats = (size_t)r->fn_.P;
    *row0 = r->fn_.params + first * *row_floats;
    return FDSP_OK;
}

int fx_resynth_table(FxBank* fx, bool gain, size_t first, size_t count, float** row0, size_t* row_floats) {
    auto* r = dynamic_cast<ResynthFx*>(fx);
    if (!r) return api_fail(FDSP_EINVAL, "fdsp_resynth_set_band / _gain: not a resynthesizer bank");
    const RsConst& c = r->c_;
    if (c.proc == RS_FN) return api_fail(FDSP_ENOTSUP, "fdsp_resynth_set_band / _gain: a closure bank has no stock tables (fdsp_resynth_set_params)");
    if (c.proc != (gain ? FDSP_RESYNTH_GAIN : FDSP_RESYNTH_BAND))
        return api_fail(FDSP_EINVAL, gain ? "fdsp_resynth_set_gain: the bank's processor is not FDSP_RESYNTH_GAIN" : "fdsp_resynth_set_band: the bank's processor is not FDSP_RESYNTH_BAND");
    const size_t rows = (size_t)c.rows;
    if (first > rows || count > rows - first) return api_fail(FDSP_EINVAL, "fdsp_resynth_set_band / _gain: rows out of range (one row per instance with per_instance, else the single row 0)");
    *row_floats = (size_t)c.O * (gain ? (size_t)(c.N / 2 + 1) : 2);
    *row0 = (gain ? (float*)c.gain : (float*)c.band) + first * *row_floats;
    return FDSP_OK;
}

// the sizes that follow from the capacity, the outputs c.C and the instances; then the bank (c.C, c.NT, c.I and the routing or the terms set)
static int cv_finish(CvConst c, size_t V, const fdsp_convolve_spec& sp, hipStream_t s, std::unique_ptr<FxBank>* out) {
    c.B = cv_block_length(sp.max_len);
    while ((1 << c.logB) < c.B) c.logB++;
    c.rows = sp.per_instance ? (int)V : 1;
    c.Pcap = (int)((sp.max_len + c.B - 1) / c.B);
    c.Hcap = (size_t)(c.Pcap + 1) * c.B;
    // blocks per chunk: the Z buffer within 256 MiB where the bank is large, at least one tile of the tail kernel
    size_t KB = ((size_t)256 << 20) / (V * (size_t)c.C * (c.B + 1) * sizeof(float2));
    KB = KB < 8 ? 8 : (KB > 64 ? 64 : KB);
    c.KB = (int)KB;
    c.R = c.Pcap + c.KB;
    c.Rx = 1;
    while (c.Rx < (c.KB + 1) * c.B) c.Rx <<= 1;
    c.invN = 1.0f / (float)(2 * c.B);
    auto r = std::make_unique<ConvolveFx>(c, sp.flush_denormals, V, sp.max_len);
    if (int rc = r->init(sp.response, sp.len, s)) return rc;
    *out = std::move(r);
    return FDSP_OK;
}
int fx_convolve(size_t instances, const fdsp_convolve_spec& sp, int inputs, const int* source, hipStream_t s, std::unique_ptr<FxBank>* out) {
    CvConst c{};
    c.C = c.NT = sp.channels;
    cv_set_routing(c, source ? inputs : sp.channels, source, source != nullptr);   // source NULL: fdsp_convolve_create, the plain kernel sequence
    return cv_finish(c, instances, sp, s, out);
}
int fx_convolve_matrix(size_t instances, const fdsp_convolve_spec& sp, int inputs, int outputs, const int* term_input, const int* term_output, hipStream_t s,
                       std::unique_ptr<FxBank>* out) {
    CvConst c{};
    c.C = outputs;
    c.NT = sp.channels;
    c.I = inputs;
    c.sum = 1;
    for (int t = 0; t < c.NT; t++) {
        c.tin[t] = term_input[t];
        c.tfirst[term_output[t] + 1] = t + 1;   // term_output is non-decreasing and names every output: the last term of o ends at t + 1
    }
    for (int o = outputs + 1; o <= CV_MAX_CH; o++) c.tfirst[o] = c.NT;
    return cv_finish(c, instances, sp, s, out);
}
int fx_convolve_check(FxBank* fx, size_t len, size_t first, size_t count) {
    auto* r = dynamic_cast<ConvolveFx*>(fx);
    if (!r) return api_fail(FDSP_EINVAL, "fdsp_convolve_set_response: not a convolver bank");
    return r->check_response(len, first, count);
}
int fx_convolve_response(FxBank* fx, const float* h, size_t len, size_t first, size_t count, hipStream_t s) {
    return static_cast<ConvolveFx*>(fx)->set_response(h, len, first, count, s);
}
int fx_convolve_block_length(size_t max_len) { return cv_block_length(max_len); }

}  // namespace fd

extern "C" int fdsp_resynth_tables(int window_length, float* h_hann, float* h_twiddles) {
    const int N = window_length;
    if (N < 4 || N > 8192 || (N & (N - 1)) != 0) return fd::api_fail(FDSP_EINVAL, "fdsp_resynth_tables: window_length takes a power of two from 4 to 8192");
    fd::rs_tables(N, h_hann, nullptr, h_twiddles);
    return FDSP_OK;
}
