// fd_seq.hpp -- the reference Sequencer's clock arithmetic, host + device, shared by the voice scheduler's kernels (fd_device.hpp
// render_sched_body, a lane is a voice: one event per voice, or a voice plays one note of a score after another;
// render_score_notes_body, a lane is a note), by the steps they are built from (fd_seq_steps.hpp) and by the CPU checks
// tests/host/check_score_blocks.hip and check_score_notes.hip.  Follows src/sequencer.rs: ready_to_active :584-605, process :838-951,
// fade_in / fade_out :122-216, Fade::at :51-56, smooth5 / sine_ease math.rs:418-420,453-458.  Needs fd_math.hpp only.
#pragma once

#include "fd_math.hpp"

namespace fd {

FD_HD float smooth5f(float x) { return ((x * 6.0f - 15.0f) * x + 10.0f) * x * x * x; }
FD_HD float sine_easef(float x) {  // Bhaskara's approximation, math.rs:453-458
    constexpr float PI_F = (float)3.14159265358979323846, HALF_PI_F = (float)(3.14159265358979323846 * 0.5);
    constexpr float D = (float)(5.0 * 3.14159265358979323846 * 3.14159265358979323846);
    x = x * HALF_PI_F;
    return 16.0f * x * (PI_F - x) / (D - 4.0f * x * (PI_F - x));
}
FD_HD float fade_at(int ease, float x) { return ease == 0 ? sine_easef(x) : smooth5f(x); }
FD_HD long long round_index(double x) {  // `round(x) as usize`: half away from zero, negative / NaN -> 0
    double r = __builtin_round(x);
    return r > 0.0 ? (r < 4.0e18 ? (long long)r : (long long)4.0e18) : 0;
}

// What one Sequencer::process block of `size` frames starting at clock `time` does with an event (start, end, fade_in, fade_out):
// whether the event plays in it at all, its frame window [start_index, end_index) inside the block -- the unit's own process()
// block -- and the state of the two fades at the window's first frame.  The fade indices count from the window's start, like
// the reference's (they index the event's own buffer).  The phases are re-derived from the f64 clock in every block and then
// accumulated in f32 (cur += d per faded frame).
struct SeqBlock {
    bool act;
    long long start_index, end_index;
    bool fin_on;          // fade_in :122-167: frames k < fin_end_i of the window are scaled by fade_at(ease, fin_cur + k * fin_d)
    long long fin_end_i;
    float fin_cur, fin_d;
    bool fout_on;         // fade_out :169-216: frames fout_i <= k < end_index by fade_at(ease, 1 - (fout_cur + (k - fout_i) * fout_d))
    long long fout_i;
    float fout_cur, fout_d;
};
FD_HD SeqBlock seq_block(double e_start, double e_end, double e_fin, double e_fout, double time, int size, double sample_rate) {
    SeqBlock b;
    const double sd = 1.0 / sample_rate;  // Sequencer::set_sample_rate :752-753
    const double end_time = time + sd * (double)size;
    const double threshold = end_time - sd * 0.5;                       // ready_to_active :586
    b.act = e_start < threshold && !(e_end <= time + 0.5 * sd);         // :588, :861
    b.start_index = e_start <= time ? 0 : round_index((e_start - time) * sample_rate);
    b.end_index = size;
    if (!(e_end >= end_time)) {
        long long r = round_index((e_end - time) * sample_rate);
        b.end_index = r < size ? r : size;
    }
    b.act = b.act && b.end_index > b.start_index;
    b.fin_on = false;
    b.fin_end_i = 0;
    b.fin_cur = 0.0f;
    b.fin_d = 0.0f;
    {
        const double fade_end = e_start + e_fin;
        if (b.act && e_fin > 0.0 && fade_end > time) {
            b.fin_on = true;
            b.fin_end_i = fade_end >= end_time ? b.end_index : round_index((fade_end - time) / sd);
            b.fin_cur = (float)(((time + (double)b.start_index * sd) - e_start) / (fade_end - e_start));
            b.fin_d = (float)(sd / e_fin);
        }
    }
    b.fout_on = false;
    b.fout_i = 0;
    b.fout_cur = 0.0f;
    b.fout_d = 0.0f;
    {
        const double fade_start = e_end - e_fout;
        if (b.act && e_fout > 0.0 && fade_start < end_time) {
            b.fout_on = true;
            b.fout_i = fade_start <= time ? 0 : round_index((fade_start - time) / sd);
            b.fout_cur = (float)(((time + (double)b.fout_i * sd) - fade_start) / (e_end - fade_start));
            b.fout_d = (float)(sd / e_fout);
        }
    }
    return b;
}

// ---- scores: a voice plays the notes of its sorted range one after the other (end_k <= start_{k+1}) -----------------------
// Nothing but the clock says where a voice stands.  At a block (or tick) starting at `time`:
//   a note is over             iff  end <= time + 0.5 sd           (the reference's end_of_event test, :861 / :797)
//   a note has already begun   iff  start < time - 0.5 sd          (the PREVIOUS block's ready_to_active test: `time` was its end_time)
// so the voice's current note is the first one that is not over, and a note that is active without having begun starts here.
FD_HD bool seq_note_over(double e_end, double time, double sd) { return e_end <= time + 0.5 * sd; }
FD_HD bool seq_note_begun(double e_start, double time, double sd) { return e_start < time - 0.5 * sd; }
FD_HD bool seq_note_ready(double e_start, double end_time, double sd) { return e_start < end_time - sd * 0.5; }
// first note of [lo, hi) that is not over at `time` (ends are non-decreasing within a voice)
FD_HD int seq_first_live(const double* ends, int lo, int hi, double time, double sd) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (seq_note_over(ends[mid], time, sd)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ---- scores, one lane per note (render_score_notes_body): which note of a voice owns the write-back ------------------------
// The launch's blocks are 64 frames long (1 in tick mode), counted from the launch start and ragged at the end; the clock of a
// block is the launch's clock advanced by ONE f64 addition of sd * size per block before it -- never time0 + b * 64 * sd, which
// differs in the last bits.  These walk it that way from a block [t, ...) whose clock is `time`.
// Does the note render a frame in the rest of the launch?  *late: it is not ready before the launch's last block ends (then
// neither is any later note of its voice).  A note renders in a block iff seq_block says so; in tick mode iff it is ready and
// not over at the tick.
FD_HD bool seq_note_renders(double e_start, double e_end, double time, size_t t, size_t T, bool tick, double sd, double sample_rate,
                            bool* late) {
    *late = false;
    bool ready = false;
    while (t < T) {
        if (seq_note_over(e_end, time, sd)) return false;  // ... and stays over
        const int size = tick ? 1 : (int)((T - t) < 64 ? (T - t) : 64);
        const double end_time = time + sd * (double)size;
        if (seq_note_ready(e_start, end_time, sd)) {
            if (tick || seq_block(e_start, e_end, 0.0, 0.0, time, size, sample_rate).act) return true;
            ready = true;
        }
        time = end_time;
        t += (size_t)size;
    }
    *late = !ready;
    return false;
}
// Note j of a voice whose range ends at hi rendered its last frame in the block [t, ...) with clock `time`: is it the LAST note of the
// voice to render in this launch?  One look at note j + 1 in practice; the loop exists for notes of zero length, which never render.
FD_HD bool seq_note_owns_state(const double* ev, size_t N, int j, int hi, double time, size_t t, size_t T, bool tick, double sd,
                               double sample_rate) {
    for (int q = j + 1; q < hi; q++) {
        bool late;
        if (seq_note_renders(ev[q], ev[N + q], time, t, T, tick, sd, sample_rate, &late)) return false;
        if (late) break;
    }
    return true;
}

// A score on the device (fdsp_bank_set_score), sorted by (voice, start): note_begin[V + 1] is the CSR index of the voices'
// ranges, ev[4][N] = start, end, fade_in, fade_out (f64 seconds), fade[N] the curves, params[nparams][N] the notes' rows for
// the nparams slots param_slot[] (f32 slots, indices in visit order).  Passed to the kernels by value.
struct ScoreData {
    const int* note_begin;
    const double* ev;
    const int* fade;
    const float* params;
    const int* param_slot;
    int N, nparams;
};
constexpr int SCORE_MAX_PARAMS = 16;

}  // namespace fd
