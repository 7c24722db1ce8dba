// fd_seq_steps.hpp -- the steps of the voice scheduler that its kernels share, each written ONCE, host + device: the lane-per-voice
// body of the events and the score kernels (fd_device.hpp render_sched_body), the lane-per-note body (render_score_notes_body) and the
// CPU checks tests/host/check_score_blocks.hip and check_score_notes.hip, which compile this very source.  These are the steps that
// have to match the reference Sequencer bit for bit (src/sequencer.rs process :838-951, tick :769-836, fade_in / fade_out :122-216):
// the begin_block / PH_SIMD / end_simd / PH_REM sequence of a unit's own process() block, the f32 accumulation of the fade phases, the
// tick-mode fades from the f64 clock, the packed block with its rollback, and what beginning a note means.  The clock arithmetic they
// work on is fd_seq.hpp.  A step is templated over the unit type G and force-inlined; it calls nothing that is device-only: where the
// frames come from and where they go (HBM, the LDS tile of the fused mix) stays in the kernel bodies or comes in as a callable.
#pragma once

#include "fd_nodes.hpp"
#include "fd_seq.hpp"

namespace fd {

// ---- a note's window: the part [si, ei) of a Sequencer block that the note plays in, the unit's own process() block ----------
struct SeqWindow {
    int full;                // frames of the window's whole 8-frame SIMD items: PH_SIMD below, PH_REM from there on
    float fin_cur, fout_cur; // the fade phases, re-derived from the clock by seq_block and accumulated in f32 per faded frame
};
// the window of n = ei - si frames begins
template <class G>
FD_HD SeqWindow seq_window_begin(G& g, const SeqBlock& w, int n) {
    SeqWindow s{n & ~7, w.fin_cur, w.fout_cur};
    g.begin_block(n);
    if (s.full == 0) g.end_simd();
    return s;
}
// frame kk of the window: fi[G::IN] -> fo[G::OUT], faded
template <class G>
FD_HD void seq_window_frame(G& g, const SeqBlock& w, SeqWindow& s, int ease, int kk, const float* fi, float* fo) {
    if (kk < s.full) g.template step<PH_SIMD>(fi, fo); else g.template step<PH_REM>(fi, fo);
    if (kk + 1 == s.full) g.end_simd();
    if (w.fin_on && kk < w.fin_end_i) {
        const float e = fade_at(ease, s.fin_cur);
#pragma unroll
        for (int c = 0; c < G::OUT; c++) fo[c] *= e;
        s.fin_cur += w.fin_d;
    }
    // `kk < w.end_index` compares an index of the WINDOW with an index of the BLOCK.  Kept on purpose: it is the comparison the kernels
    // have always made (it never cuts a fade-out short: kk < ei - si <= end_index), and no comparison of this step may move.
    if (w.fout_on && kk >= w.fout_i && kk < w.end_index) {
        const float e = fade_at(ease, 1.0f - s.fout_cur);
#pragma unroll
        for (int c = 0; c < G::OUT; c++) fo[c] *= e;
        s.fout_cur += w.fout_d;
    }
}

// ---- tick mode: the two fades of the frame at clock `time`, straight from the f64 clock (Sequencer::tick :769-836) ------------
template <int NO>
FD_HD void seq_tick_fades(double e_start, double e_end, double e_fin, double e_fout, int ease, double time, float* fo) {
    if (e_fin > 0.0) {
        const float f = (float)((time - e_start) / ((e_start + e_fin) - e_start));
        if (f < 1.0f) {
            const float e = fade_at(ease, f);
#pragma unroll
            for (int c = 0; c < NO; c++) fo[c] *= e;
        }
    }
    if (e_fout > 0.0) {
        const float f = (float)((time - (e_end - e_fout)) / (e_end - (e_end - e_fout)));
        if (f > 0.0f) {
            const float e = fade_at(ease, 1.0f - f);
#pragma unroll
            for (int c = 0; c < NO; c++) fo[c] *= e;
        }
    }
}

// ---- the steady block: a plain process(size) of the unit, no window edge and no fade inside it ---------------------------------
// The whole SIMD items take the packed two-frame path (step2: the same arithmetic per frame); if a packed shortcut left its exact
// domain (tripped), the unit goes back to the snapshot and the items are redone frame by frame.  load(c, i) is input channel c of the
// block's frame i, put(c, i, x) takes output channel c of frame i (a redone frame is put a second time).
template <class G, class Load, class Put>
FD_HD void seq_steady_block(G& g, int size, Load&& load, Put&& put) {
    constexpr int NI = G::IN, NO = G::OUT;
    const int full = size & ~7;
    g.begin_block(size);
    const G snap = g;
    for (int i = 0; i < full; i += 2) {
        v2f pi[NI > 0 ? NI : 1], po[NO];
#pragma unroll
        for (int c = 0; c < NI; c++) pi[c] = v2f{load(c, i), load(c, i + 1)};
        g.template step2<PH_SIMD>(pi, po);
#pragma unroll
        for (int c = 0; c < NO; c++) {
            put(c, i, po[c].x);
            put(c, i + 1, po[c].y);
        }
    }
    if (__builtin_expect(g.tripped(), 0)) {  // a packed-path shortcut left its exact domain: redo the block
        g = snap;
        for (int i = 0; i < full; i++) {
            float fi[NI > 0 ? NI : 1], fo[NO];
#pragma unroll
            for (int c = 0; c < NI; c++) fi[c] = load(c, i);
            g.template step<PH_SIMD>(fi, fo);
#pragma unroll
            for (int c = 0; c < NO; c++) put(c, i, fo[c]);
        }
    }
    g.end_simd();
    for (int i = full; i < size; i++) {
        float fi[NI > 0 ? NI : 1], fo[NO];
#pragma unroll
        for (int c = 0; c < NI; c++) fi[c] = load(c, i);
        g.template step<PH_REM>(fi, fo);
#pragma unroll
        for (int c = 0; c < NO; c++) put(c, i, fo[c]);
    }
}

// ---- a note begins: a fresh unit with the voice's hash and parameters and the note's row (lifecycle ops 1 and 2) ------------------
// `row` is a visitor that writes the note's parameters over the slots the score names
template <class G, class Row>
FD_HD void seq_note_begin(G& g, Row& row, double sample_rate) {
    g.visit(row);
    g.update(sample_rate);
    g.reset();
}

}  // namespace fd
