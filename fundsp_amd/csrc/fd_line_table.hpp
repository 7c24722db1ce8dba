// fd_line_table.hpp -- host: the per-line part of a line network's device table, written once for the row types of both families (FdnxInst of
// fd_fdnx.hpp, FbInst of fd_fbdelay.hpp): N lines `delay [>> fir] [>> F] [* g]` of an FdnxDesc at a sample rate.  Included by the two units
// that build tables (fd_fdnx.hip, fd_fbdelay.hip) and not by fd_fdnx.hpp: the coefficients need fd_nodes.hpp, which the effect banks do not.
#pragma once

#include <cmath>

#include "fd_fdnx.hpp"
#include "fd_math.hpp"
#include "fd_nodes.hpp"   // svf_coefs

namespace fd {

struct LineSpan { int longest, shortest; };   // ring lengths (delay + 1) over all rows and lines; shortest < 0: a ring would exceed 2^18 slots

// len, w, co and g of every row of `tab` (d.per_instance ? instances : 1 rows of d.lines lines); what else a row or the constants hold is
// the family's
template <class Row>
LineSpan line_table_fill(const FdnxDesc& d, size_t instances, double sample_rate, std::vector<Row>& tab) {
    const size_t P = d.per_instance ? instances : 1;
    const int N = d.lines;
    tab.assign(P, Row{});
    const float sr = (float)sample_rate;   // the filters' coefficients are computed in F = f32 (filter.rs:35-38, svf.rs:236-239)
    LineSpan span{0, 1 << 30};
    for (size_t p = 0; p < P; p++) {
        Row& e = tab[p];
        for (int k = 0; k < N; k++) {
            const size_t i = p * N + k;
            const double samples = std::round(d.delay[i] * sample_rate);   // Delay::new / set_sample_rate (delay.rs:104-112)
            if (!(samples + 1.0 <= (double)(1 << 18))) return {0, -1};     // (before the conversion: a count past int has no int value)
            e.len[k] = (int)samples + 1;
            span.longest = e.len[k] > span.longest ? e.len[k] : span.longest;
            span.shortest = e.len[k] < span.shortest ? e.len[k] : span.shortest;
            for (int j = 0; j < d.taps; j++) e.w[j][k] = d.w[i * d.taps + j];
            if (d.filter == FDNX_LOWPOLE) {
                e.co[0][k] = expf_musl(-F32_TAU * d.cutoff[i] / sr);   // Lowpole::set_cutoff (filter.rs:35-38)
                e.co[1][k] = 1.0f - e.co[0][k];                         // (1 - coeff) as tick computes it (:65)
            } else if (d.filter == FDNX_SVF) {
                const SvfCoefs s = svf_coefs(d.svf_mode, sr, d.cutoff[i], d.q[i], d.gain.empty() ? 1.0f : d.gain[i]);
                e.co[0][k] = s.a1; e.co[1][k] = s.a2; e.co[2][k] = s.a3; e.co[3][k] = s.m0; e.co[4][k] = s.m1; e.co[5][k] = s.m2;
            }
            e.g[k] = d.has_gain ? d.line_gain[i] : 1.0f;
        }
    }
    return span;
}

// slots per ring: the power of two, at least 256, that holds the longest ring
inline int line_ring_cap(int longest) {
    int cap = 256;
    while (cap < longest) cap <<= 1;
    return cap;
}

}  // namespace fd
