// fd_resynth_fn.hpp -- the processing closure of a resynthesizer bank as a C++ functor, compiled at run time (fdsp_resynth_fn_create).
//
// resynth::<I, O, _>(window, |fft| ...) (resynth.rs:227-233) takes the caller's closure.  Here the closure is a type in namespace fd, given as
// source text in the PER-BIN form, and compiled by the library's own hiprtc next to this header (fd_jit.hip, the library's flags,
// -ffp-contract=off; the flush-to-zero flags for a bank created with flush_denormals):
//
//     struct Gate {
//         static constexpr int PARAMS = 1;   // f32 values per instance, set from the host between launches
//         static constexpr int STATE  = 0;   // f32 values per (instance, bin) that live from frame to frame; 0.0 at creation and after reset
//         template <class W> static __device__ void bin(W& fft, int i) {
//             const Cf x = fft.at(0, i);
//             if (x.re * x.re + x.im * x.im >= fft.param(0)) fft.set(0, i, x);
//         }
//     };
//
// bin(fft, i) is called once per frame and bin i in 0 .. fft.bins() - 1.  It stands for the Rust closure
//     |fft| for i in 0..fft.bins() { BODY(i) }
// whose body reads any INPUT bin and writes OUTPUT bin i only.  The view W mirrors FftWindow (resynth.rs:38-155):
//     inputs(), outputs(), length(), bins()
//     at(channel, j)          input bin j of a channel, ANY j (shifts, mirrors and blurs are gathers); out of range (channel or j) gives zero
//     set(channel, i, value)  writes the CALLING bin only: another i, or a channel out of range, is dropped, so no functor can store out of
//                             bounds.  An output bin that is not set is zero (clear_output, resynth.rs:361)
//     frequency(j)            (sr as f32 / N as f32) * j as f32 -- the value the stock `band` processor uses
//     sample_rate(), latency(), time(), time_at(j), delta_time(), windows_per_second()   in f64, operation for operation as resynth.rs:53-97;
//                             `samples` of the frame that completes at sample count k H is k H
//     param(p)                parameter p of the instance (0.0 out of range)
//     state(s)                a reference to value s of the calling bin's own state
// NOT in the contract, and absent rather than half-built: writing another bin than one's own (dropped), reading outputs (there is no
// at_output), state shared between bins.
// With STATE > 0 the frames of one instance are processed in increasing order (an FnMut closure sees them in that order); with STATE == 0
// all frames of a chunk are independent.  PARAMS and STATE must equal the spec's (static_assert in the generated module).
//
// The stock closures as functors (1 -> 1; further channels repeat the line with other channel numbers):
//     struct Pass { static constexpr int PARAMS = 0, STATE = 0;
//         template <class W> static __device__ void bin(W& fft, int i) { fft.set(0, i, fft.at(0, i)); } };
//     struct Band { static constexpr int PARAMS = 2, STATE = 0;   // (lo, hi) in Hz
//         template <class W> static __device__ void bin(W& fft, int i) {
//             const float f = fft.frequency(i);
//             if (fft.param(0) <= f && f <= fft.param(1)) fft.set(0, i, fft.at(0, i)); } };
//     template <int BINS> struct Gain { static constexpr int PARAMS = BINS, STATE = 0;   // one gain per bin
//         template <class W> static __device__ void bin(W& fft, int i) { fft.set(0, i, fft.at(0, i) * fft.param(i)); } };
//
// Device layout.  The stock path does a frame's forward and inverse transform in one unit (k_rs_frames); a closure may read every input and
// write every output, so the closure path is cut at the spectra, per chunk:
//     k_rs_forward  one unit per (frame, instance, INPUT): windowed load, N/2-point transform, split -> X [instance][frame][input][bin]
//     rs_process    this header's kernel around the functor.  STATE == 0: one lane per (instance, frame, bin).  STATE > 0: one lane per
//                   (instance, bin), walking the chunk's frames in order with its state in registers, loaded from and stored to
//                   [instance][bin][STATE].  It writes Y [instance][frame][output][bin]
//     k_rs_inverse  one unit per (frame, instance, OUTPUT): fix_negative, the reversal, the N-point transform, / N -> the frame ring
// between the stock path's k_rs_input and k_rs_ola.  Forward and inverse are ahead-of-time kernels made of the device functions k_rs_frames
// uses, so a spectrum has the same bits on both paths.  The workspace X | Y takes instances x Fc x (I + O) x (N/2 + 1) x 8 bytes, Fc the
// frames per chunk.  With R the frame ring's slots (fd_resynth.hpp)
//     Fc = clamp(floor(R x O x N / (2 x (I + O) x (N/2 + 1))), 2, R - 4),   chunk length Lmax = (Fc - 1) x N/4,
// so the workspace does not exceed the frame ring (R x instances x O x N x 4 bytes) but at the floor of two frames (only where I > 3 O on
// an 8-slot ring).  Any split of a launch gives the same bits.
#pragma once

namespace fd {

// the process kernel's argument block (host and device; X and Y hold (re, im) pairs of f32)
struct RsFnArgs {
    const float2* x;                   // [V][Fc][I][N/2 + 1]
    float2* y;                         // [V][Fc][O][N/2 + 1]
    const float* params;               // [V][P]
    float* state;                      // [V][N/2 + 1][S]
    const unsigned long long* samples; // [1] samples processed before this chunk
    const float* fstep;                // [1] (sr as f32) / (N as f32)
    const float* srf;                  // [1] sr as f32
    unsigned long long V;
    int N, I, O, P, Fc, L, Fmax;
};

#ifdef __HIPCC_RTC__

struct Cf {
    float re, im;
};
__device__ __forceinline__ Cf operator+(Cf a, Cf b) { return Cf{a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ Cf operator-(Cf a, Cf b) { return Cf{a.re - b.re, a.im - b.im}; }
// Complex32 * Complex32 and Complex32 * f32 as num-complex writes them (no FMA: the module builds with -ffp-contract=off)
__device__ __forceinline__ Cf operator*(Cf a, Cf b) { return Cf{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ Cf operator*(Cf a, float g) { return Cf{a.re * g, a.im * g}; }

template <int S>
struct RsView {
    const Cf* x_;          // this (instance, frame)'s input spectra [I][bins]
    Cf* y_;                // ... and output spectra [O][bins]
    const float* p_;       // the instance's parameters
    float st_[S > 0 ? S : 1];
    unsigned long long samples_;
    float fstep_, srf_;
    int N_, I_, O_, P_, bin_;
    unsigned set_;         // outputs this bin has written

    __device__ int inputs() const { return I_; }
    __device__ int outputs() const { return O_; }
    __device__ int length() const { return N_; }
    __device__ int bins() const { return (N_ >> 1) + 1; }
    __device__ Cf at(int channel, int j) const {
        return ((unsigned)channel < (unsigned)I_ && (unsigned)j < (unsigned)bins()) ? x_[(size_t)channel * bins() + j] : Cf{0.0f, 0.0f};
    }
    __device__ void set(int channel, int i, Cf value) {
        if (i != bin_ || (unsigned)channel >= (unsigned)O_) return;
        y_[(size_t)channel * bins() + i] = value;
        set_ |= 1u << channel;
    }
    __device__ float frequency(int j) const { return fstep_ * (float)j; }
    __device__ double sample_rate() const { return (double)srf_; }
    __device__ double latency() const { return (double)N_ / (double)srf_; }
    __device__ double time() const { return (double)(samples_ - ((unsigned long long)N_ >> 1)) / (double)srf_; }
    __device__ double time_at(int j) const { return (double)(samples_ - (unsigned long long)N_ + (unsigned long long)j) / (double)srf_; }
    __device__ double windows_per_second() const { return 4.0 * (double)srf_ / (double)N_; }
    __device__ double delta_time() const { return (double)N_ / (4.0 * (double)srf_); }
    __device__ float param(int p) const { return (unsigned)p < (unsigned)P_ ? p_[p] : 0.0f; }
    __device__ float& state(int s) { return st_[(unsigned)s < (unsigned)S ? s : 0]; }
};

// frame f of the chunk for one (instance, bin): the functor, then zeros for the outputs it left unset
template <class F, int S>
__device__ __forceinline__ void rs_process_frame(const RsFnArgs& a, RsView<S>& w, size_t v, int f, unsigned long long k) {
    const int NB = (a.N >> 1) + 1;
    w.x_ = (const Cf*)a.x + (v * a.Fc + f) * (size_t)a.I * NB;
    w.y_ = (Cf*)a.y + (v * a.Fc + f) * (size_t)a.O * NB;
    w.samples_ = k * (unsigned long long)(a.N >> 2);
    w.set_ = 0;
    F::bin(w, w.bin_);
    for (int o = 0; o < a.O; o++)
        if (!(w.set_ >> o & 1u)) w.y_[(size_t)o * NB + w.bin_] = Cf{0.0f, 0.0f};
}

template <class F>
__device__ __forceinline__ void rs_process_body(const RsFnArgs& a) {
    constexpr int S = F::STATE;
    const int NB = (a.N >> 1) + 1, H = a.N >> 2;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long S0 = *a.samples, k0 = S0 / H + 1;
    RsView<S> w;
    w.fstep_ = *a.fstep;
    w.srf_ = *a.srf;
    w.N_ = a.N; w.I_ = a.I; w.O_ = a.O; w.P_ = a.P;
    if constexpr (S == 0) {
        if (idx >= (size_t)a.V * a.Fmax * NB) return;
        w.bin_ = (int)(idx % NB);
        const int f = (int)((idx / NB) % a.Fmax);
        const size_t v = idx / ((size_t)NB * a.Fmax);
        const unsigned long long k = k0 + f;
        if (k * H > S0 + (unsigned long long)a.L || k < 4) return;   // no frame completes there (k_rs_frames' `live`)
        w.p_ = a.params + v * (size_t)a.P;
        w.st_[0] = 0.0f;
        rs_process_frame<F, S>(a, w, v, f, k);
    } else {
        if (idx >= (size_t)a.V * NB) return;
        w.bin_ = (int)(idx % NB);
        const size_t v = idx / NB;
        w.p_ = a.params + v * (size_t)a.P;
        float* st = a.state + idx * S;
#pragma unroll
        for (int s = 0; s < S; s++) w.st_[s] = st[s];
        for (int f = 0; f < a.Fmax; f++) {
            const unsigned long long k = k0 + f;
            if (k * H > S0 + (unsigned long long)a.L || k < 4) continue;
            rs_process_frame<F, S>(a, w, v, f, k);
        }
#pragma unroll
        for (int s = 0; s < S; s++) st[s] = w.st_[s];
    }
}

#endif  // __HIPCC_RTC__

}  // namespace fd
