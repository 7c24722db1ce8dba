// fd_fxbank.hpp -- the effect banks: banks of one stock node per instance instead of a voice graph of slots -- the Hadamard networks
// (reverb_stereo, reverb4_stereo, the generic `fdn`: fd_fdn.hpp), reverb3_stereo (fd_reverb3.hpp), the filtered / per-instance networks
// (fd_fdnx.hpp), the feedback delay banks (fd_fbdelay.hpp), the resynthesizer (fd_resynth.hpp) and the convolver (fd_convolve.hpp).  fd_capi.hip keeps the bank handle (stream, events, pan weights, launch options)
// and the public constructors' argument checks; what a family allocates, configures, copies and launches is behind FxBank (fd_fxbank.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

#include <memory>
#include <string>
#include <vector>

#include "../../include/fundsp_hip.h"
#include "fd_fdn.hpp"   // FdnBus

namespace fd {

int api_fail(int code, const std::string& msg);  // fd_capi.hip: records fdsp_last_error() for this thread

// Work goes to the stream given; the caller owns the waits around it.  int results are FDSP_* codes with fdsp_last_error() set.
struct FxBank {
    virtual ~FxBank() = default;   // frees every device buffer the instance allocated
    virtual int inputs() const = 0;
    virtual int outputs() const = 0;
    virtual FdnBus* bus() { return nullptr; }   // nullptr: the resynthesizer and the convolver, which render through fdsp_bank_process only
    // a network changes nothing unless the rate changes and reconfigures transactionally: on failure it keeps its rate and state
    virtual int set_sample_rate(double sr, hipStream_t stream) = 0;
    virtual hipError_t reset(hipStream_t stream) = 0;
    // a new instance that continues exactly where this one stands (state copied on `stream`, bus included)
    virtual int clone(hipStream_t stream, std::unique_ptr<FxBank>* out) = 0;
    virtual void render(const float* in, float* out, size_t T, size_t fstride, int layout, int tick, bool capturing, hipStream_t stream) = 0;
    // The fused mix-down (fdsp_bank_process_mix): the family renders into a scratch of its own, chunk by chunk, and leaves the groups'
    // partial mixes in part[groups][mix channels][T] (panw = [2][pstride] weights: FDSP_MIX_PAN, one output; else NULL); the caller runs the
    // tree.  The default is a family without one (the resynthesizer, the convolver).  The scratch is sized by mix_reserve only -- never by
    // render_mix, which a capture may record -- and lives until the bank goes; mix_reserved tells whether a launch of T frames fits.
    virtual bool has_mix() const { return false; }
    virtual bool mix_reserved(size_t) const { return false; }
    virtual int mix_reserve(size_t) { return api_fail(FDSP_ENOTSUP, "this effect bank has no fused mix-down"); }
    virtual void render_mix(const float*, float*, size_t, size_t, int, int, const float*, size_t, hipStream_t) {}
};

// fd_fxmix.hip: planar [V][C][xstride], frames 0 .. n-1 -> columns t0 .. t0+n-1 of the groups' partial mixes part[groups][C or 2][T]
void fx_launch_mix_groups(const float* x, size_t V, int C, size_t xstride, size_t n, float* part, size_t T, size_t t0, const float* panw,
                          size_t pstride, hipStream_t stream);
// frames t0 .. t0+n-1 of voice-minor [channels][T][V] -> planar [V][channels][dstride], frames 0 .. n-1
void fx_launch_stage_in(const float* src, float* dst, size_t V, size_t T, int channels, size_t t0, size_t n, size_t dstride, hipStream_t stream);
void fx_launch_copy_rows(const float* src, size_t sstride, float* dst, size_t dstride, size_t rows, size_t n, hipStream_t stream);

// The factories build and initialise an instance on `stream`.  The arguments are checked by the caller; what can still fail is the
// kernels' delay rule at the creation rate (44.1 kHz but for fx_fdn_network and fx_feedback_delay) and the allocation.
// sections 1: reverb_stereo(room_size, time, damping), 2: reverb4_stereo(room_size, time)
int fx_reverb_stereo(size_t instances, int sections, double room_size, double time, double damping, hipStream_t stream, std::unique_ptr<FxBank>* out);
// reverb4_stereo_delays(delays, time): `delays` = [32] f32 seconds, or [instances][32] with per_instance (fd_fdn.hpp "PER INSTANCE")
int fx_reverb4_delays(size_t instances, const float* delays, int per_instance, double time, hipStream_t stream, std::unique_ptr<FxBank>* out);
// fdsp_reverb4_set_delays: refuses what is not such a bank (`fx` may be NULL), rows out of range, and a delay that is negative, not a number,
// under 128 samples or beyond the bank's ring capacity before anything changes; then uploads the rows and resets their instances on
// `stream` and waits for it (the host array is borrowed)
int fx_reverb4_set_delays(FxBank* fx, const float* rows, size_t first, size_t count, hipStream_t stream);
int fx_fdn(size_t instances, int lines, const double* delays, int taps, const float* weights, int inputs, int outputs, hipStream_t stream,
           std::unique_ptr<FxBank>* out);
// svf_mode < 0: lowpole_hz(cutoff) in the loop, else FixedSvf(svf_mode, cutoff, q, gain)
int fx_reverb3_stereo(size_t instances, double time, double diffusion, int svf_mode, float cutoff, float q, float gain, hipStream_t stream,
                      std::unique_ptr<FxBank>* out);
int fx_fdn_network(size_t instances, const fdsp_fdn_network& net, double sample_rate, hipStream_t stream, std::unique_ptr<FxBank>* out);
// the feedback delay banks (fd_fbdelay.hpp; the description checked by the caller but for the delay rules at `sample_rate`)
int fx_feedback_delay(size_t instances, const fdsp_feedback_delay& net, double sample_rate, hipStream_t stream, std::unique_ptr<FxBank>* out);
int fx_resynth(size_t instances, const fdsp_resynth_spec& spec, hipStream_t stream, std::unique_ptr<FxBank>* out);
// a closure bank (fd_resynth_fn.hpp): the functor's module is compiled and loaded before anything is allocated; _compile alone needs no device
int fx_resynth_fn(size_t instances, const fdsp_resynth_fn_spec& spec, hipStream_t stream, std::unique_ptr<FxBank>* out);
int fx_resynth_fn_compile(const fdsp_resynth_fn_spec& spec, std::shared_ptr<const std::vector<char>>* code);
// fdsp_resynth_set_params: checks the bank (`fx` may be NULL) and the instances; the device address of row `first` and the floats per row
int fx_resynth_params(FxBank* fx, size_t first, size_t count, float** row0, size_t* row_floats);
// fdsp_resynth_set_band / _gain: checks the bank (`fx` may be NULL) and the rows; the device address of row `first` and the floats per row
int fx_resynth_table(FxBank* fx, bool gain, size_t first, size_t count, float** row0, size_t* row_floats);
// source NULL: the plain bank of fdsp_convolve_create; else the routed bank of fdsp_convolve_routed_create (`inputs` and the `channels`
// entries of `source` checked by the caller; read during the call only)
int fx_convolve(size_t instances, const fdsp_convolve_spec& spec, int inputs, const int* source, hipStream_t stream, std::unique_ptr<FxBank>* out);
// the summing bank of fdsp_convolve_matrix_create: spec.channels terms (response rows), term t reading input term_input[t] into output
// term_output[t] (both tables and the counts checked by the caller; read during the call only)
int fx_convolve_matrix(size_t instances, const fdsp_convolve_spec& spec, int inputs, int outputs, const int* term_input, const int* term_output,
                       hipStream_t stream, std::unique_ptr<FxBank>* out);
// fdsp_convolve_set_response: _check refuses what is not a convolver bank (`fx` may be NULL), a length beyond the capacity and rows out of
// range before anything is touched; _response uploads [count][channels][len] for rows first .. first+count-1, transforms the partitions on
// `stream` and clears the history (the caller waits for the stream: the host array is borrowed)
int fx_convolve_check(FxBank* fx, size_t len, size_t first, size_t count);
int fx_convolve_response(FxBank* fx, const float* h_response, size_t len, size_t first, size_t count, hipStream_t stream);
int fx_convolve_block_length(size_t max_len);   // the block length B a bank of this response capacity uses (fd_convolve.hpp)

}  // namespace fd
