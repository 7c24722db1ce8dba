// tests/host/check_score_notes.hip -- host-side check (hipcc, host only) of the two ways to execute a score (fd_device.hpp):
//   render_sched_body        a lane is a VOICE: it walks the launch block by block and plays its notes one after the other (render_score_body);
//   render_score_notes_body  a lane is a NOTE: it starts from the voice's slots as they stand at the launch start, walks only the blocks
//                            its note lives in, and the last note of the voice that rendered a frame (fd_seq.hpp seq_note_owns_state)
//                            stores the voice's state to a staging image that is committed after the launch.
// Both walks are restated here on the CPU over a real node type, the FM + SVF voice, with the shared clock arithmetic of fd_seq.hpp; what
// happens inside a note's window, in a tick and when a note begins is NOT restated: it is the kernels' own source, fd_seq_steps.hpp.  They
// run over random scores -- legato pairs, several notes in one block, notes of zero length (one directly behind the last rendered note
// of a voice), notes carried across a split, off-grid times -- in one launch and in split launches, process and tick.  Every sample and
// the slot image of every voice after every launch must be bit-equal.  Also pinned: the block clock is the ACCUMULATED one
// (time += sd * size per block); time0 + b * 64 * sd differs from it in the last bits.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#define FD_HOST_ONLY 1
#include "fd_seq_steps.hpp"
using namespace fd;

using G = Pipe<Pipe<Unop<Pipe<Constant<1>, Sine>, UAddScalar>, Sine>, FixedSvf>;  // the FM + SVF voice (fm_svf)
constexpr double SR = 48000.0;

struct HImage {  // every slot word of a voice, in visit order (what VStore<true> writes)
    std::vector<uint32_t> w;
    void f(float& x, FieldKind, const char*) { uint32_t u; memcpy(&u, &x, 4); w.push_back(u); }
    void fi(float& x, FieldKind k, const char* n, int) { f(x, k, n); }
    void u32(uint32_t& x, FieldKind, const char*) { w.push_back(x); }
    void u64(uint64_t& x, FieldKind, const char*) { w.push_back((uint32_t)x); w.push_back((uint32_t)(x >> 32)); }
    void enter(int) {}
    void leave() {}
};
struct HSetRow {  // VSetRow: the note's row over the named f32 slots
    const std::vector<int>* slot_of;
    const float* row;
    int slot;
    void put(float& x) {
        for (size_t j = 0; j < slot_of->size(); j++)
            if ((*slot_of)[j] == slot) x = row[j];
        slot++;
    }
    void f(float& x, FieldKind, const char*) { put(x); }
    void fi(float& x, FieldKind, const char*, int) { put(x); }
    void u32(uint32_t&, FieldKind, const char*) { slot++; }
    void u64(uint64_t&, FieldKind, const char*) { slot += 2; }
    void enter(int) {}
    void leave() {}
};
struct HFirstParam {  // the first f32 PARAM slot
    int slot = 0, found = -1;
    void put(FieldKind k) { if (k == PARAM && found < 0) found = slot; slot++; }
    void f(float&, FieldKind k, const char*) { put(k); }
    void fi(float&, FieldKind k, const char*, int) { put(k); }
    void u32(uint32_t&, FieldKind, const char*) { slot++; }
    void u64(uint64_t&, FieldKind, const char*) { slot += 2; }
    void enter(int) {}
    void leave() {}
};

struct Score {  // sorted by (voice, start)
    int V = 0;
    std::vector<int> note_begin, fade;
    std::vector<double> ev;  // [4][N]
    std::vector<float> rows;
    std::vector<int> slot_of;
    size_t N() const { return fade.size(); }
};
static void begin_note(G& g, const Score& sc, int j) {
    HSetRow row{&sc.slot_of, &sc.rows[(size_t)j * sc.slot_of.size()], 0};
    seq_note_begin(g, row, SR);
}
// one tick of note j at clock `time`: the unit's tick and the kernels' tick-mode fades
static float tick_frame(G& g, const Score& sc, int j, double time) {
    const size_t N = sc.N();
    float fi[1] = {0.0f}, fo[1] = {0.0f};
    g.template step<PH_TICK>(fi, fo);
    seq_tick_fades<1>(sc.ev[j], sc.ev[N + j], sc.ev[2 * N + j], sc.ev[3 * N + j], sc.fade[j], time, fo);
    return fo[0];
}
// the note's own sub-block [si, ei) of a launch block starting at frame t0, by the kernels' window steps
static void window_frames(G& g, const Score& sc, int j, const SeqBlock& w, size_t t0, float* out) {
    const int si = (int)w.start_index, ei = (int)w.end_index;
    SeqWindow win = seq_window_begin(g, w, ei - si);
    for (int kk = 0; kk < ei - si; kk++) {
        float fi[1] = {0.0f}, fo[1] = {0.0f};
        seq_window_frame(g, w, win, sc.fade[j], kk, fi, fo);
        out[t0 + (size_t)(si + kk)] = fo[0];
    }
}

// ---- a lane is a voice (render_score_body, its frame-by-frame walk) --------------------------------------------------------------
static void serial_voice(G& g, const Score& sc, int v, double time0, size_t T, bool tick, float* out) {
    const size_t N = sc.N();
    const double sd = 1.0 / SR, inf_ = __builtin_huge_val();
    const int ne = sc.note_begin[v + 1];
    int k = seq_first_live(sc.ev.data() + N, sc.note_begin[v], ne, time0, sd);
    auto start = [&](int j) { return j < ne ? sc.ev[j] : inf_; };
    auto end = [&](int j) { return j < ne ? sc.ev[N + j] : -inf_; };
    double time = time0;
    if (!tick) {
        for (size_t t0 = 0; t0 < T; t0 += 64) {
            const int size = (int)((T - t0) < 64 ? (T - t0) : 64);
            const double end_time = time + sd * (double)size;
            while (k < ne && seq_note_over(end(k), time, sd)) k++;
            for (;;) {  // the current note's window, then every further note that is ready in this block
                if (k < ne) {
                    const SeqBlock w = seq_block(sc.ev[k], sc.ev[N + k], sc.ev[2 * N + k], sc.ev[3 * N + k], time, size, SR);
                    if (w.act) {
                        if (!seq_note_begun(sc.ev[k], time, sd)) begin_note(g, sc, k);
                        window_frames(g, sc, k, w, t0, out);
                    }
                }
                if (!seq_note_ready(start(k + 1), end_time, sd)) break;
                k++;
            }
            time = end_time;
        }
    } else {
        for (size_t t = 0; t < T; t++) {
            const double end_time = time + sd;
            while (k < ne && seq_note_over(end(k), time, sd)) k++;
            if (seq_note_ready(start(k), end_time, sd) && !seq_note_over(end(k), time, sd)) {
                if (!seq_note_begun(sc.ev[k], time, sd)) begin_note(g, sc, k);
                out[t] = tick_frame(g, sc, k, time);
            }
            time = end_time;
        }
    }
}

// ---- a lane is a note (render_score_notes_body) ---------------------------------------------------------------------------------
// returns true when the note owns the voice's write-back; *g is then the state to store
static bool note_lane(G& g, const Score& sc, int v, int j, double time0, size_t T, bool tick, float* out) {
    const size_t N = sc.N();
    const double sd = 1.0 / SR;
    const double e_start = sc.ev[j], e_end = sc.ev[N + j];
    if (seq_note_over(e_end, time0, sd)) return false;
    double time = time0;
    size_t t0 = 0;
    for (;;) {
        if (t0 >= T) return false;
        const int size = tick ? 1 : (int)((T - t0) < 64 ? (T - t0) : 64);
        const double end_time = time + sd * (double)size;
        if (seq_note_ready(e_start, end_time, sd)) break;
        time = end_time;
        t0 += (size_t)size;
    }
    bool rendered = false;
    double time_last = time;
    size_t t_last = t0;
    if (!tick) {
        for (; t0 < T && !seq_note_over(e_end, time, sd); t0 += 64) {
            const int size = (int)((T - t0) < 64 ? (T - t0) : 64);
            const double end_time = time + sd * (double)size;
            const SeqBlock w = seq_block(e_start, e_end, sc.ev[2 * N + j], sc.ev[3 * N + j], time, size, SR);
            if (w.act) {
                if (!seq_note_begun(e_start, time, sd)) begin_note(g, sc, j);
                window_frames(g, sc, j, w, t0, out);
                rendered = true;
                time_last = time;
                t_last = t0;
            }
            time = end_time;
        }
    } else {
        for (; t0 < T && !seq_note_over(e_end, time, sd); t0++) {
            const double end_time = time + sd;
            if (seq_note_ready(e_start, end_time, sd)) {
                if (!seq_note_begun(e_start, time, sd)) begin_note(g, sc, j);
                out[t0] = tick_frame(g, sc, j, time);
                rendered = true;
                time_last = time;
                t_last = t0;
            }
            time = end_time;
        }
    }
    return rendered && seq_note_owns_state(sc.ev.data(), N, j, sc.note_begin[v + 1], time_last, t_last, T, tick, sd, SR);
}

// ---- scores --------------------------------------------------------------------------------------------------------------------
static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static double rnd01() { return (double)rnd() / 16777216.0; }
static int rndi(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

// voices of short and long notes; `cuts`: launch boundaries (frames) the crafted voice 0 is built around
static Score make_score(int V, size_t T, const std::vector<size_t>& cuts, int first_param) {
    struct Note { double s, e, fi, fo; int fade; float row; };
    std::vector<std::vector<Note>> per(V);
    const double sd = 1.0 / SR;
    for (int v = 0; v < V; v++) {
        double pos = (double)rndi(0, 90);  // frames
        if (v == 0 && !cuts.empty()) {
            // a note carried across the first cut, legato into a short one; then, ahead of the second cut, a rendered note with a note of
            // zero length directly behind it and nothing else before the cut: the zero-length note must not take the write-back
            const double c0 = (double)cuts[0], c1 = cuts.size() > 1 ? (double)cuts[1] : (double)T;
            per[v].push_back({(c0 - 37.3) * sd, (c0 + 21.0) * sd, 5.0 * sd, 9.0 * sd, 1, 300.0f});
            per[v].push_back({(c0 + 21.0) * sd, (c0 + 24.0) * sd, 0.0, 0.0, 0, 410.0f});
            per[v].push_back({(c1 - 30.0) * sd, (c1 - 11.5) * sd, 0.0, 4.0 * sd, 1, 150.0f});
            per[v].push_back({(c1 - 11.5) * sd, (c1 - 11.5) * sd, 0.0, 0.0, 1, 999.0f});
            pos = c1 + 3.0;
        }
        while (pos < (double)T + 40.0) {
            const int kind = rndi(0, 9);
            double dur = kind == 0 ? 0.0 : kind < 6 ? (double)rndi(1, 12) : kind < 9 ? (double)rndi(13, 90) : (double)rndi(91, 260);
            double s = pos, e = pos + dur;
            if (rndi(0, 2) == 0) { s += rnd01() * 0.8 - 0.4; if (s < 0) s = 0; }   // off-grid
            if (rndi(0, 2) == 0) e += rnd01() * 0.8 - 0.4;
            if (e < s) e = s;
            Note n{s * sd, e * sd, 0.0, 0.0, rndi(0, 1), (float)(80.0 + 800.0 * rnd01())};
            const double d = n.e - n.s;
            if (rndi(0, 1)) n.fi = d * rnd01();
            if (rndi(0, 1)) n.fo = d * rnd01();
            per[v].push_back(n);
            const int gap = rndi(0, 5);
            pos = e + (gap < 3 ? 0.0 : gap < 5 ? (double)rndi(1, 3) : (double)rndi(20, 200));  // legato, a few frames, a pause
            if (gap < 3 && !per[v].empty()) pos = e;  // legato: the next start IS this end (the same double after the division below)
        }
        // the overlap rule on the doubles themselves
        for (size_t i = 1; i < per[v].size(); i++)
            if (per[v][i].s < per[v][i - 1].e) per[v][i].s = per[v][i - 1].e, per[v][i].e = per[v][i].e < per[v][i].s ? per[v][i].s : per[v][i].e;
        for (Note& n : per[v]) {
            const double d = n.e - n.s;
            if (n.fi > d) n.fi = d;
            if (n.fo > d) n.fo = d;
        }
    }
    Score sc;
    sc.V = V;
    sc.slot_of = {first_param};
    size_t N = 0;
    for (auto& p : per) N += p.size();
    sc.ev.resize(4 * N);
    sc.note_begin.push_back(0);
    size_t j = 0;
    for (int v = 0; v < V; v++) {
        for (const Note& n : per[v]) {
            sc.ev[j] = n.s; sc.ev[N + j] = n.e; sc.ev[2 * N + j] = n.fi; sc.ev[3 * N + j] = n.fo;
            sc.fade.push_back(n.fade);
            sc.rows.push_back(n.row);
            j++;
        }
        sc.note_begin.push_back((int)j);
    }
    return sc;
}

static std::vector<G> fresh_voices(int V) {
    std::vector<G> gs(V);
    for (int v = 0; v < V; v++) {
        G& g = gs[v];
        g.init();
        g.x.x.x.x.value[0] = 220.0f + 10.0f * v;  // the modulator's frequency: the slot the rows overwrite
        g.x.x.scalar = 220.0f;
        g.y.cutoff = 1500.0f; g.y.q = 2.0f; g.y.gain = 1.0f;
        g.update(SR);
        uint64_t h = g.ping(true, G::ID);
        g.ping(false, h ^ (0x9e3779b97f4a7c15ULL * (uint64_t)(v + 1)));
        g.reset();
    }
    return gs;
}
static std::vector<uint32_t> image(G& g) { HImage im; g.visit(im); return im.w; }

static int run_case(const char* name, int V, size_t T, const std::vector<size_t>& launches, bool tick, uint32_t seed) {
    rng_state = seed;
    HFirstParam fp;
    { G g; g.visit(fp); }
    std::vector<size_t> cuts;
    { size_t t = 0; for (size_t n : launches) { t += n; if (t < T) cuts.push_back(t); } }
    const Score sc = make_score(V, T, cuts, fp.found);
    std::vector<G> a = fresh_voices(V), b = fresh_voices(V);
    const double sd = 1.0 / SR;
    double time = 0.0;
    int bad = 0, zero_len = 0, carried = 0, owners = 0;
    for (size_t n : launches) {
        std::vector<float> oa((size_t)V * n, 0.0f), ob((size_t)V * n, 0.0f);
        for (int v = 0; v < V; v++) serial_voice(a[v], sc, v, time, n, tick, &oa[(size_t)v * n]);
        std::vector<G> stage = b;  // the staging image; flagged voices are committed after the launch
        std::vector<char> flag(V, 0);
        for (int v = 0; v < V; v++)
            for (int j = sc.note_begin[v]; j < sc.note_begin[v + 1]; j++) {
                G g = b[v];  // every lane loads the slots as they stand at the launch start
                zero_len += sc.ev[j] == sc.ev[sc.N() + j];
                carried += seq_note_begun(sc.ev[j], time, sd) && !seq_note_over(sc.ev[sc.N() + j], time, sd);
                if (note_lane(g, sc, v, j, time, n, tick, &ob[(size_t)v * n])) {
                    if (flag[v]) { printf("%s: two notes own voice %d\n", name, v); bad++; }
                    stage[v] = g;
                    flag[v] = 1;
                    owners++;
                }
            }
        for (int v = 0; v < V; v++)
            if (flag[v]) b[v] = stage[v];
        int ds = 0, di = 0;
        for (size_t i = 0; i < oa.size(); i++) ds += memcmp(&oa[i], &ob[i], 4) != 0;
        for (int v = 0; v < V; v++) di += image(a[v]) != image(b[v]);
        if (ds || di) printf("%s: launch of %zu frames at clock %.9f: %d samples, %d voice images differ\n", name, n, time, ds, di);
        bad += ds + di;
        if (!tick) for (size_t t = 0; t < n; t += 64) time += sd * (double)(n - t < 64 ? n - t : 64);
        else for (size_t t = 0; t < n; t++) time += sd;
    }
    printf("%-28s %zu notes, %d zero-length, %d carried in, %d write-backs: %s\n", name, sc.N(), zero_len, carried, owners, bad ? "MISMATCH" : "equal");
    if (!zero_len || !owners || (launches.size() > 1 && !carried)) { printf("%s: the score misses a case it must contain\n", name); bad++; }
    return bad;
}

int main() {
    int bad = 0;
    {  // the clock trap: 96 000 frames at 48 kHz, block clocks accumulated vs multiplied
        const double sd = 1.0 / 48000.0;
        double acc = 0.25;
        int differ = 0;
        for (int b = 0; b < 1500; b++) {
            differ += acc != 0.25 + (double)b * 64.0 * sd;
            acc += sd * 64.0;
        }
        printf("block clocks of a 96 000-frame launch: %d of 1500 differ between accumulation and multiplication\n", differ);
        if (!differ) { printf("the clock trap is not pinned\n"); bad++; }
    }
    const size_t T = 64 * 11 + 29;
    bad += run_case("process, one launch", 6, T, {T}, false, 1u);
    bad += run_case("process, split", 6, T, {64, 128, 64 * 3, 64, T - 64 * 7}, false, 2u);
    bad += run_case("process, split, other seed", 7, T, {64 * 2, 64, 64 * 5, T - 64 * 8}, false, 3u);
    bad += run_case("tick, one launch", 5, T, {T}, true, 4u);
    bad += run_case("tick, split", 5, T, {50, 77, 300, T - 427}, true, 5u);
    printf("%s\n", bad ? "MISMATCH" : "all equal");
    return bad != 0;
}
