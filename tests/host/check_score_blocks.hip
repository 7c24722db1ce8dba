// tests/host/check_score_blocks.hip -- host-side check (hipcc, host only, its own main): the clock arithmetic the score kernels share with the
// events kernels (fundsp_amd/csrc/fd_seq.hpp: seq_block, seq_first_live, seq_note_over / _begun / _ready) and the note-advance rule of
// the lane-per-voice body (fd_device.hpp render_sched_body with ScoreNotes), walked on the CPU over random scores -- block by block and tick by
// tick, in one launch and in split launches -- next to the oracle's Sequencer (oracle/o_sequencer.c).  What happens to a frame inside a note's
// window, in a tick and when a note begins is the kernels' own source: the steps of fundsp_amd/csrc/fd_seq_steps.hpp.  The WALK itself --
// load_note, the advance over notes that are over, the look loop, open() -- is still a restatement of render_sched_body's (the kernel's takes
// its notes through a policy and works on a wave): a change of the walk has to be made in both places, and this check pins this copy of it.
// Every note's unit is a constant: note k outputs k + 1, so a frame's sample says which note owns it and carries the bits of its fade factors.
// The walk also counts how often each note is begun (row written, update, reset): exactly once for a note that plays, right at its first frame --
// except a note that is already running when a walk starts in its middle (a launch boundary), which must continue instead.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#define FD_HOST_ONLY 1
#include "fd_seq_steps.hpp"
extern "C" {
#include "fundsp_oracle.h"
}
using namespace fd;

struct Score {
    int V;
    std::vector<int> nb;              // [V + 1]
    std::vector<double> ev;           // [4][N]
    std::vector<int> fade;            // [N]
    int N() const { return (int)fade.size(); }
};
struct Walk {  // one voice's lane state between launches: nothing but what the slots would hold
    std::vector<int> begun;           // per note: how often it was begun
    std::vector<long> first_frame;    // per note: the first frame it played (-1: never)
    std::vector<long> begun_frame;    // per note: the frame index at which it was begun
};
// The unit the kernels' steps (fd_seq_steps.hpp) run over here: a constant that says which note owns the frame.  Beginning it -- the
// reset() at the end of seq_note_begin -- is what the walk counts.
struct NoteUnit {
    static constexpr int IN = 0, OUT = 1;
    Walk* w;
    int note;    // the lane's current note
    long frame;  // where it is begun
    template <class V> void visit(V&) {}
    void update(double) {}
    void reset() { w->begun[note]++; w->begun_frame[note] = frame; }
    void begin_block(int) {}
    void end_simd() {}
    template <int PH> void step(const float*, float* out) { out[0] = (float)(note + 1); }
};
struct NoRow {};  // these scores have no parameter rows

static unsigned rs = 12345;
static double rnd() { rs = rs * 1664525u + 1013904223u; return (double)(rs >> 8) * (1.0 / 16777216.0); }

// one launch of `T` frames of voice v from clock time0, the way render_sched_body walks it; out[T] gets the voice's samples
static double walk_launch(const Score& sc, int v, size_t T, double time0, double sr, bool process, float* out, Walk& w, long frame0) {
    const int N = sc.N(), ne = sc.nb[v + 1];
    const double sd = 1.0 / sr, inf_ = __builtin_huge_val();
    int k = seq_first_live(sc.ev.data() + N, sc.nb[v], ne, time0, sd);
    double e_start, e_end, e_fin, e_fout;
    int ease;
    auto load_note = [&](int j) {
        const bool on = j < ne;
        e_start = on ? sc.ev[j] : inf_;
        e_end = on ? sc.ev[N + j] : -inf_;
        e_fin = on ? sc.ev[2 * N + j] : 0.0;
        e_fout = on ? sc.ev[3 * N + j] : 0.0;
        ease = on ? sc.fade[j] : 1;
    };
    NoteUnit u{&w, 0, 0};
    NoRow row;
    auto begin_note = [&](int j, long frame) { u.note = j; u.frame = frame; seq_note_begin(u, row, sr); };
    auto played = [&](int j, long frame) { if (w.first_frame[j] < 0) w.first_frame[j] = frame; };
    load_note(k);
    double time = time0;
    if (process) {
        for (size_t t0 = 0; t0 < T; t0 += 64) {
            const int size = (int)((T - t0) < 64 ? (T - t0) : 64);
            const double end_time = time + sd * (double)size;
            while (k < ne && seq_note_over(e_end, time, sd)) load_note(++k);
            SeqBlock b = seq_block(e_start, e_end, e_fin, e_fout, time, size, sr);
            int si = 0, ei = 0;
            SeqWindow win{0, 0.0f, 0.0f};
            auto open = [&]() {  // the window of the current note; the note is begun where the window is found, what counts is its first frame
                si = b.act ? (int)b.start_index : 0;
                ei = b.act ? (int)b.end_index : 0;
                if (b.act) {
                    if (!seq_note_begun(e_start, time, sd)) begin_note(k, frame0 + (long)t0 + si);
                    win = seq_window_begin(u, b, ei - si);
                }
            };
            open();
            bool look = true;
            for (int i = 0; i < size; i++) {
                while (look && i >= ei) {
                    const double next_start = k + 1 < ne ? sc.ev[k + 1] : inf_;
                    look = seq_note_ready(next_start, end_time, sd);
                    if (!look) break;
                    load_note(++k);
                    b = seq_block(e_start, e_end, e_fin, e_fout, time, size, sr);
                    open();
                }
                float x = 0.0f;
                if (i >= si && i < ei) {
                    u.note = k;
                    played(k, frame0 + (long)t0 + i);
                    seq_window_frame(u, b, win, ease, i - si, nullptr, &x);
                }
                out[t0 + i] = x;
            }
            time = end_time;
        }
    } else {
        for (size_t t = 0; t < T; t++) {
            const double end_time = time + sd;
            while (k < ne && seq_note_over(e_end, time, sd)) load_note(++k);
            const bool act = seq_note_ready(e_start, end_time, sd) && !seq_note_over(e_end, time, sd);
            float x = 0.0f;
            if (act) {
                if (!seq_note_begun(e_start, time, sd)) begin_note(k, frame0 + (long)t);
                played(k, frame0 + (long)t);
                u.note = k;
                u.step<PH_TICK>(nullptr, &x);
                seq_tick_fades<1>(e_start, e_end, e_fin, e_fout, ease, time, &x);
            }
            out[t] = x;
            time = end_time;
        }
    }
    return time;
}

// a random score: per voice 0 .. 7 notes, durations from below one sample to several blocks, gaps from 0 (legato) up, times off the sample grid
static Score random_score(int V, size_t T, double sr) {
    Score sc;
    sc.V = V;
    sc.nb.assign(V + 1, 0);
    std::vector<double> st, en, fi, fo;
    std::vector<bool> legato;
    for (int v = 0; v < V; v++) {
        const int n = (int)(rnd() * 8);
        double t = rnd() < 0.3 ? 0.0 : rnd() * 90.0;  // in samples
        for (int j = 0; j < n; j++) {
            const double r = rnd();
            double dur = r < 0.2 ? 0.2 + rnd() * 2.0 : r < 0.6 ? 3.0 + floor(rnd() * 18.0) : r < 0.8 ? 64.0 : 20.0 + floor(rnd() * 300.0);
            if (rnd() < 0.5) t += rnd() * 0.4 - 0.2;
            if (t < 0.0) t = 0.0;
            const double s = t / sr, e = (t + dur) / sr, d = e - s;
            const double q = rnd();
            st.push_back(s);
            en.push_back(e);
            fi.push_back(q < 0.3 ? 0.0 : q < 0.5 ? d : d * rnd());
            const double q2 = rnd();
            fo.push_back(q2 < 0.3 ? 0.0 : q2 < 0.5 ? d : d * rnd());
            sc.fade.push_back(rnd() < 0.5 ? 0 : 1);
            t += dur;
            const double g = rnd();
            legato.push_back(g < 0.35);   // the NEXT note starts at exactly this note's end
            if (g >= 0.35) t += g < 0.7 ? rnd() * 6.0 : rnd() * 200.0;
        }
        sc.nb[v + 1] = (int)sc.fade.size();
    }
    const int N = sc.N();
    sc.ev.resize(4 * (size_t)N);
    for (int j = 0; j < N; j++) {
        sc.ev[j] = st[j];
        sc.ev[N + j] = en[j];
        sc.ev[2 * N + j] = fi[j];
        sc.ev[3 * N + j] = fo[j];
    }
    // in order: legato pairs share the boundary's exact bits, every other pair satisfies end <= next start, fades fit the (possibly shortened) note
    for (int v = 0; v < V; v++)
        for (int j = sc.nb[v]; j < sc.nb[v + 1]; j++) {
            if (j > sc.nb[v] && (legato[j - 1] || sc.ev[j] < sc.ev[N + j - 1])) sc.ev[j] = sc.ev[N + j - 1];
            if (sc.ev[N + j] < sc.ev[j]) sc.ev[N + j] = sc.ev[j];
            const double d = sc.ev[N + j] - sc.ev[j];
            if (sc.ev[2 * N + j] > d) sc.ev[2 * N + j] = d;
            if (sc.ev[3 * N + j] > d) sc.ev[3 * N + j] = d;
        }
    (void)T;
    return sc;
}

int main() {
    int bad = 0;
    long notes_total = 0, notes_played = 0, frames_played = 0;
    const double rates[] = {48000.0, 44100.0};
    for (int round = 0; round < 24; round++) {
        const double sr = rates[round & 1];
        const int V = 9;
        const size_t T = 64 * 9 + 21;
        const bool process = (round & 2) == 0;
        const Score sc = random_score(V, T, sr);
        const int N = sc.N();
        // the oracle: one Sequencer event per note, a constant unit worth (note index + 1)
        oseq* s = o_seq_new(0, 1, sr);
        for (int j = 0; j < N; j++) {
            const float val = (float)(j + 1);
            if (o_seq_push(s, sc.ev[j], sc.ev[N + j], sc.fade[j], sc.ev[2 * N + j], sc.ev[3 * N + j], o_constant(1, &val)) < 0) { printf("push failed\n"); return 2; }
        }
        std::vector<float> mix(T), per((size_t)(N ? N : 1) * T, 0.0f);
        o_seq_render(s, T, process ? 1 : 0, nullptr, mix.data(), per.data());
        const double t_oracle = o_seq_time(s);
        o_seq_free(s);
        // the walk: once in one launch, once in launches of (64 * 5, 64 * 4, 21), once in ragged launches
        const size_t splits[3][4] = {{T, 0, 0, 0}, {64 * 5, 64 * 4, 21, 0}, {64 * 3, 64 * 2, 64 * 4, 21}};
        for (int sp = 0; sp < 3; sp++) {
            int diff = 0, lifecycle = 0;
            double t_walk = 0.0;
            for (int v = 0; v < V; v++) {
                std::vector<float> want(T, 0.0f), got(T, 0.0f);
                for (int j = sc.nb[v]; j < sc.nb[v + 1]; j++)
                    for (size_t t = 0; t < T; t++) {
                        uint32_t bits;
                        memcpy(&bits, &per[(size_t)j * T + t], 4);
                        if (bits != 0) want[t] = per[(size_t)j * T + t];
                    }
                Walk w;
                w.begun.assign(N, 0);
                w.first_frame.assign(N, -1);
                w.begun_frame.assign(N, -1);
                double time = 0.0;
                size_t done = 0;
                for (int l = 0; l < 4 && splits[sp][l]; l++) {
                    time = walk_launch(sc, v, splits[sp][l], time, sr, process, got.data() + done, w, (long)done);
                    done += splits[sp][l];
                }
                t_walk = time;
                for (size_t t = 0; t < T; t++) diff += memcmp(&want[t], &got[t], 4) != 0;
                if (sp == 0) {
                    for (size_t t = 0; t < T; t++) frames_played += want[t] != 0.0f;
                    for (int j = sc.nb[v]; j < sc.nb[v + 1]; j++) notes_total++, notes_played += w.first_frame[j] >= 0;
                }
                for (int j = sc.nb[v]; j < sc.nb[v + 1]; j++) {
                    const bool plays = w.first_frame[j] >= 0;
                    if (plays ? (w.begun[j] != 1 || w.begun_frame[j] != w.first_frame[j]) : (w.begun[j] > 1)) lifecycle++;
                }
            }
            if (diff || lifecycle || t_walk != t_oracle) {
                printf("round %d (%s, sr %.0f) split %d: %d frames differ, %d notes begun wrongly, clock %.17g vs %.17g\n", round, process ? "process" : "tick", sr, sp, diff,
                       lifecycle, t_walk, t_oracle);
                bad++;
            }
        }
    }
    printf("%ld notes, %ld of them played, %ld sounding frames\n", notes_total, notes_played, frames_played);
    if (notes_played < 300 || frames_played < 20000) { printf("the scores exercise too little\n"); return 2; }
    printf("%s\n", bad ? "MISMATCH" : "all equal");
    return bad != 0;
}
