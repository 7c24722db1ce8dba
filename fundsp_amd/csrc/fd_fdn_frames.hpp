// fd_fdn_frames.hpp -- the steps of a 64-frame block that the lane = FRAME feedback kernels share: k_fdn_render_frames and
// k_fdn_frames_generic (fd_fdn.hip), k_fdn_frames_filtered (fd_fdnx.hip) and k_fb_frames (fd_fbdelay.hip); device functions, and at the end
// the host-side launch ladder.  One wave renders one instance, lane = frame,
// the lines of the network in registers; every delay is at least two blocks (128 samples), so all ring reads of a block are known at its head.
// These are the steps that have to match the reference bit for bit (the order of the FIR terms, the butterfly stage order, tick against
// process in the joins, the mirror zone): each is written ONCE here, and a kernel is a sequence of them with its own parts in between (the
// pan fold and the series join of the reverbs, the filter of the filtered networks).  A step is templated on what the kernels are
// templated on (lines NL, FIR order K, the extent N of the register array) and force-inlined: no step branches on its caller.
//
// Where a line's parameters come from stays the kernel's business.  A step that needs them takes an accessor with `len(k)` (the ring
// length of line k) and `w(j, k)` (FIR weight j of line k): kernel arguments in SGPRs (FdnConst) or a row of the per-instance table
// (FdnxInst, scalar loads).
#pragma once

#include "fd_fdn.hpp"

namespace fd {

// floats per LDS row of a line.  History rows: the K - 1 carried delay outputs | d[0..63].  Feedback rows: fb[-1] | fb[0..63]; the
// filtered kernel also hands a block's 64 frames to its serial lanes in [4..67] (16-byte aligned).
constexpr int HS = 68;

// the wave-local LDS hand-off: the rows belong to one wave, so no workgroup barrier
__device__ __forceinline__ void fdn_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The instance's rings as a buffer resource: buffer_load / buffer_store take a VGPR offset (lane * 4, the same for every access), an
// SGPR offset (the line's base + the block's slot, scalar arithmetic) and no 64-bit VALU address math.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t fdn_rings(const FdnState& s, size_t inst, size_t ring_stride) {
    return __builtin_amdgcn_make_buffer_rsrc(s.rings + inst * ring_stride, 0, (int)(ring_stride * sizeof(float)), 0x00020000);
}

// frames of the block at t0: 64, or what is left of a launch that is no multiple of 64 frames
__device__ __forceinline__ int fdn_block_size(size_t T, size_t t0) { return (int)((T - t0) < 64 ? (T - t0) : 64); }

// carry-in of line `k` (the lanes below the number of lines take one each): Fir::v[1..K-1] (v1 = the older, v2 = the newer of a Fir<U3>; a
// Fir<U2> keeps its one sample in v2) and Feedback::value, into slots 0 .. of the line's rows
template <int K>
__device__ __forceinline__ void fdn_state_load(const FdnState& s, size_t inst, int k, float* hist, float* fbr) {
    if (K == 3) hist[k * HS + 0] = (s.v1 + inst * 32)[k];
    if (K >= 2) hist[k * HS + K - 2] = (s.v2 + inst * 32)[k];
    fbr[k * HS + 0] = (s.fb + inst * 32)[k];
}

// ... and back at the end of the launch
template <int K>
__device__ __forceinline__ void fdn_state_store(const FdnState& s, size_t inst, int k, const float* hist, const float* fbr) {
    if (K == 3) (s.v1 + inst * 32)[k] = hist[k * HS + 0];
    if (K >= 2) (s.v2 + inst * 32)[k] = hist[k * HS + K - 2];
    (s.fb + inst * 32)[k] = fbr[k * HS + 0];
}

// Ring reads of the block whose first frame is written at `wpn`, issued one block AHEAD (consumed after the current block's arithmetic,
// which hides the HBM latency).  Frame 0 reads the slot written len - 1 frames ago (delay.rs:116-124); the 64 slots from there on are
// contiguous (the mirror zone), in bounds for every lane, and lanes past a ragged end read values nobody uses.
template <int NL, class P>
__device__ __forceinline__ void fdn_ring_fetch(float (&dn)[NL], __amdgpu_buffer_rsrc_t rings, int lane4, int cap, int wpn, const P& p) {
#pragma unroll
    for (int k = 0; k < NL; k++) {
        const int r = (wpn - (p.len(k) - 1)) & (cap - 1);
        dn[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rings, lane4, (k * (cap + 64) + r) * 4, 0));
    }
}

// Fir::tick fir.rs:57-70 of one line: the sum starts at 0.0 and takes the taps oldest first.  `row` = the line's history row at this
// lane's frame (slots n, n + 1 hold d[n-2], d[n-1] of a Fir<U3>), `d` the delay output of the frame.  K = 0: no Fir node in the line.
template <int K>
__device__ __forceinline__ float fdn_fir(const float* row, float d, float w0, float w1, float w2) {
    if (K == 0) return d;
    float acc = 0.0f;
    if (K == 3) {
        acc += w0 * row[0];
        acc += w1 * row[1];
        acc += w2 * d;
    } else if (K == 2) {
        acc += w0 * row[0];
        acc += w1 * d;
    } else {
        acc += w0 * d;
    }
    return acc;
}

// the FIR outputs of all lines: the delay outputs go to the history rows (lane n writes slot n + K - 1), then every lane reads the K - 1
// slots before its own
template <int NL, int K, class P>
__device__ __forceinline__ void fdn_fir_lines(float (&o)[NL], const float (&d)[NL], float* hist, int lane, const P& p) {
    if (K > 1) {
#pragma unroll
        for (int k = 0; k < NL; k++) hist[k * HS + K - 1 + lane] = d[k];
        fdn_wave_sync();
    }
#pragma unroll
    for (int k = 0; k < NL; k++) o[k] = fdn_fir<K>(hist + k * HS + lane, d[k], p.w(0, k), p.w(1, k), p.w(2, k));
}

// The one time-serial step of the filtered kernels (k_fdn_frames_filtered, k_fb_frames): a serial lane (lane = line) walks its line's 64
// frames through the line's filter, in place in the LDS `row`, eight frames at a time: the loads do not depend on the recurrence and run
// ahead of it, and the 64 frames never sit in registers at once.  `svf` is the lane's SvfCore (fd_nodes.hpp; a template parameter so that
// this header needs no node), which also carries the Lowpole's value in ic1eq; pc, pomc: the Lowpole's coeff and 1 - coeff.  A ragged last
// block: the filter stops where the launch does (its state after frame size - 1).
template <class Svf>
__device__ __forceinline__ void fdn_filter_walk(float* row, bool is_svf, Svf& svf, float pc, float pomc, int size) {
    if (is_svf) {   // FixedSvf::tick, the reference's operations in the reference's order (svf.rs:995-1006)
#pragma unroll 8
        for (int n = 0; n < 64; n++) {
            const float i1 = svf.ic1eq, i2 = svf.ic2eq;
            row[n] = svf.tick(row[n]);
            if (n >= size) { svf.ic1eq = i1; svf.ic2eq = i2; }
        }
    } else {        // Lowpole::tick: value = (1 - coeff) * x + coeff * value (filter.rs:64-66)
        float v = svf.ic1eq;
#pragma unroll 8
        for (int n = 0; n < 64; n++) {
            const float a = pomc * row[n];
            const float b = pc * v;
            const float nv = a + b;
            v = n < size ? nv : v;
            row[n] = nv;
        }
        svf.ic1eq = v;
    }
}

// FrameHadamard feedback.rs:35-57: in-place butterflies h = 1, 2, 4, .. < NL, (x, y) -> (x + y, x - y), over every NL-line network of the
// N registers; the scale (1.0 / sqrt(NL as f64)) as f32 (:57) is the caller's
template <int NL, int N>
__device__ __forceinline__ void fdn_hadamard(float (&h)[N]) {
    static_assert(NL >= 2 && (NL & (NL - 1)) == 0 && N % NL == 0, "Hadamard: a power of two lines per network");
#pragma unroll
    for (int st = 1; st < NL; st <<= 1)
#pragma unroll
        for (int i = 0; i < N; i++)
            if ((i & st) == 0) {
                const float x = h[i], y = h[i + st];
                h[i] = x + y;
                h[i + st] = x - y;
            }
}

// The feedback of frame n (the Hadamard outputs, scaled) goes to row slot n + 1: the ring write of frame n needs slot n, the value the
// frame before left ...
template <int N>
__device__ __forceinline__ void fdn_feedback_put(const float (&h)[N], float scale, float* fbr, int lane) {
#pragma unroll
    for (int k = 0; k < N; k++) fbr[k * HS + 1 + lane] = h[k] * scale;
    fdn_wave_sync();
}

// ... Feedback::tick: input + value (feedback.rs:130-134, 260-261), the new ring samples of lines K0 .. K1 - 1.  Line k takes channel
// k % 2 of (x0, x1): Split / MultiSplit, output i = input i % M (audionode.rs:559-562, 600-606); one channel: x1 = x0.
template <int K0, int K1, int N>
__device__ __forceinline__ void fdn_ring_input(float (&xw)[N], const float* fbr, int lane, float x0, float x1) {
#pragma unroll
    for (int k = K0; k < K1; k++) xw[k] = ((k & 1) ? x1 : x0) + fbr[k * HS + lane];
}

// Delay::tick of a block: the new sample of frame n takes slot (wp + n) mod cap of every ring (fd_fdn.hpp "Ring memory").  The common
// block is one scalar offset per line; a block whose write window wraps (one in cap / 64), touches the first 64 slots (their mirror behind
// the ring is kept) or is ragged (the last block of a launch that is no multiple of 64 frames) goes slot by slot.
template <int NL>
__device__ __forceinline__ void fdn_ring_store(const float (&xw)[NL], __amdgpu_buffer_rsrc_t rings, int lane, int lane4, int cap, int wp, int size) {
    const int cp = cap + 64;
    if (size == 64 && wp >= 64 && wp + 64 <= cap) {
#pragma unroll
        for (int k = 0; k < NL; k++) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, xw[k]), rings, lane4, (k * cp + wp) * 4, 0);
    } else if (lane < size) {
        const int pos = (wp + lane) & (cap - 1);
#pragma unroll
        for (int k = 0; k < NL; k++) {
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, xw[k]), rings, pos * 4, k * cp * 4, 0);
            if (pos < 64) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, xw[k]), rings, (cap + pos) * 4, k * cp * 4, 0);
        }
    }
}

// Join<N> / MultiJoin<M, N/M> over the first NL registers: channel j averages lines j, j + nout, ..  process() scales every term by
// z = 1 / n, then adds (audionode.rs:649-659, 706-724); tick() adds and divides (:643-648, 697-705) -- the only place where the two
// executors of these graphs differ in arithmetic.
template <int NL, int N>
__device__ __forceinline__ void fdn_join(const float (&o)[N], int nout, int tick_mode, float& y0, float& y1) {
    y1 = 0.0f;
    if (nout == 1) {
        if (tick_mode) {
            y0 = o[0];
#pragma unroll
            for (int i = 1; i < NL; i++) y0 += o[i];
            y0 = y0 / (float)NL;
        } else {
            const float z = 1.0f / (float)NL;
            y0 = o[0] * z;
#pragma unroll
            for (int i = 1; i < NL; i++) y0 += o[i] * z;
        }
    } else {
        if (tick_mode) {
            y0 = o[0]; y1 = o[1];
#pragma unroll
            for (int i = 1; i < NL / 2; i++) { y0 += o[2 * i]; y1 += o[2 * i + 1]; }
            y0 = y0 / (float)(NL / 2); y1 = y1 / (float)(NL / 2);
        } else {
            const float z = 1.0f / (float)(NL / 2);
            y0 = o[0] * z; y1 = o[1] * z;
#pragma unroll
            for (int i = 1; i < NL / 2; i++) { y0 += o[2 * i] * z; y1 += o[2 * i + 1] * z; }
        }
    }
}

// where a wave's output frames go.  layout 0: voice-minor [ch][frame][instance]; layout 1: planar [instance][ch][fstride]
struct FdnOut {
    float* out;
    size_t V, T, fstride, inst;
    int layout, lane;
};

// the bus epilogue (wet * network [& dry * multipass()], fd_fdn.hpp FdnBus; mode 2: as many outputs as inputs; x0, x1 = the block's input
// frames by channel, still in registers) and the block's output frames
__device__ __forceinline__ void fdn_output_store(const FdnOut& io, int nout, size_t t0, int size, const FdnBus& bus, float y0, float y1, float x0, float x1) {
    if (bus.mode) {
        y0 = fdn_bus(bus, y0, x0);
        y1 = fdn_bus(bus, y1, x1);
    }
    if (io.lane < size) {
        if (io.layout == 0) {
            io.out[((size_t)0 * io.T + t0 + io.lane) * io.V + io.inst] = y0;
            if (nout == 2) io.out[((size_t)1 * io.T + t0 + io.lane) * io.V + io.inst] = y1;
        } else {
            io.out[(io.inst * nout + 0) * io.fstride + t0 + io.lane] = y0;
            if (nout == 2) io.out[(io.inst * nout + 1) * io.fstride + t0 + io.lane] = y1;
        }
    }
}

// the block's last K - 1 delay outputs and its last feedback value become the next block's carry-in (row slots 0 ..)
template <int NL, int K>
__device__ __forceinline__ void fdn_block_carry(float* hist, float* fbr, int lane, int size) {
    fdn_wave_sync();
    if (lane < NL) {
        float a = 0.0f, b = 0.0f;
        if (K == 3) { a = hist[lane * HS + size]; b = hist[lane * HS + size + 1]; }
        if (K == 2) b = hist[lane * HS + size];
        const float f = fbr[lane * HS + size];
        if (K == 3) hist[lane * HS + 0] = a;
        if (K >= 2) hist[lane * HS + K - 2] = b;
        fbr[lane * HS + 0] = f;
    }
    fdn_wave_sync();
}

// Host side: one launch ladder over lines x taps for both kernel families.  KERNEL<lines, taps> with the arguments after `stream`, one wave
// per instance, four to a workgroup; K0 = the FIR order of a line without taps (the filtered kernel's 0: no Fir node; 1 where every line
// has one).
#define FD_FDN_FRAMES_GO(KERNEL, NL, K, instances, stream, ...) \
    hipLaunchKernelGGL((KERNEL<NL, K>), dim3((unsigned)(((instances) + 3) / 4)), dim3(256), 0, stream, __VA_ARGS__)
#define FD_FDN_FRAMES_TAPS(KERNEL, NL, K0, taps, instances, stream, ...)                                  \
    do {                                                                                                  \
        if ((taps) == 3) FD_FDN_FRAMES_GO(KERNEL, NL, 3, instances, stream, __VA_ARGS__);                 \
        else if ((taps) == 2) FD_FDN_FRAMES_GO(KERNEL, NL, 2, instances, stream, __VA_ARGS__);            \
        else if ((taps) == 1) FD_FDN_FRAMES_GO(KERNEL, NL, 1, instances, stream, __VA_ARGS__);            \
        else FD_FDN_FRAMES_GO(KERNEL, NL, K0, instances, stream, __VA_ARGS__);                            \
    } while (0)
#define FD_FDN_FRAMES_LAUNCH(KERNEL, K0, lines, taps, instances, stream, ...)                             \
    do {                                                                                                  \
        if ((lines) == 2) FD_FDN_FRAMES_TAPS(KERNEL, 2, K0, taps, instances, stream, __VA_ARGS__);        \
        else if ((lines) == 4) FD_FDN_FRAMES_TAPS(KERNEL, 4, K0, taps, instances, stream, __VA_ARGS__);   \
        else if ((lines) == 8) FD_FDN_FRAMES_TAPS(KERNEL, 8, K0, taps, instances, stream, __VA_ARGS__);   \
        else if ((lines) == 16) FD_FDN_FRAMES_TAPS(KERNEL, 16, K0, taps, instances, stream, __VA_ARGS__); \
        else FD_FDN_FRAMES_TAPS(KERNEL, 32, K0, taps, instances, stream, __VA_ARGS__);                    \
    } while (0)

}  // namespace fd
