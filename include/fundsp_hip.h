/*
 * fundsp_hip.h -- C ABI of the MI355X (gfx950) voice-bank engine for FunDSP leaf DSP nodes.
 *
 * Drop-in boundary.  FunDSP has no FFI of its own; the operator boundary this library replaces is the Rust
 * trait method
 *     fn process(&mut self, size: usize, input: &BufferRef, output: &mut BufferMut)   src/audionode.rs:85
 * (dyn twin AudioUnit::process, src/audiounit.rs:45) together with the lifecycle methods a node honours:
 *     reset :52, set_sample_rate :68, tick :79, set(Setting) :130, set_hash :136, ping :156, set_seed :366.
 * A *bank* is V independent voice instances of one compiled voice graph evaluated in lock-step, one wavefront
 * lane per voice.  INTEGRATION.md shows the `extern "C"` block + `impl AudioNode for HipBank` a FunDSP
 * maintainer would add on the Rust side.
 *
 * Conventions
 *  - All functions return 0 on success or a negative FDSP_E* code; fdsp_last_error() gives the message.
 *    Nothing unwinds across the ABI (AudioNode::process itself is infallible, audionode.rs:85).
 *  - Plain pointers and sizes only.  `d_*` pointers are device (HBM) pointers, `h_*` are host pointers.
 *  - A bank handle is not thread-safe but is thread-movable (AudioNode: Send, `process(&mut self)`).
 *  - Sample data is IEEE f32; internal state is f32 (prelude32, F = f32).
 *
 * Buffer layouts (`layout` argument)
 *  - FDSP_LAYOUT_VOICE_MINOR: element (channel c, frame t, voice v) at  (c*frames + t)*voices + v.
 *      Device-native: lane-consecutive addresses, no staging.
 *  - FDSP_LAYOUT_PLANAR:      element (voice v, channel c, frame t) at  (v*channels + c)*frame_stride + t.
 *      With frame_stride = 64 this is exactly an array of the reference's BufferArray/BufferRef blocks
 *      ([channel][8 x f32x8], src/buffer.rs:8-12, 356-365), one per voice; the engine transposes 64x64 tiles
 *      through LDS so HBM access stays coalesced.
 *
 * Render modes (`mode` argument)
 *  - FDSP_MODE_PROCESS: AudioNode::process semantics.  `frames` is chopped into <=64-sample blocks exactly
 *      like Wave::render (src/wave.rs:452-464); nodes that override `process` with different arithmetic
 *      (Sine: unwrapped in-block phase + f32x8 sin, src/oscillator.rs:74-86) use it for the full 8-sample
 *      SIMD items of each block and `tick` for the remainder.
 *  - FDSP_MODE_TICK: every sample through AudioNode::tick (src/audionode.rs:79).
 */
#ifndef FUNDSP_HIP_H
#define FUNDSP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FDSP_OK 0
#define FDSP_EINVAL (-1)   /* bad argument (unknown kind / parameter name / range / layout) */
#define FDSP_ENOMEM (-2)   /* device allocation failed */
#define FDSP_EDEVICE (-3)  /* HIP runtime error or no gfx950 device */
#define FDSP_ENOTSUP (-4)  /* the request is valid but this kind / bank has no kernel for it (the message says what to call instead) */

#define FDSP_LAYOUT_VOICE_MINOR 0
#define FDSP_LAYOUT_PLANAR 1

#define FDSP_MODE_PROCESS 0
#define FDSP_MODE_TICK 1

#define FDSP_MAX_BUFFER_SIZE 64 /* MAX_BUFFER_SIZE, src/lib.rs:48 */
#define FDSP_DEFAULT_SR 44100.0 /* DEFAULT_SR, src/lib.rs:42 */

/* SvfMode values for the "mode" parameter of fixed_svf / svf3 / svf4 (src/svf.rs:281-742) */
enum { FDSP_SVF_LOWPASS = 0, FDSP_SVF_HIGHPASS, FDSP_SVF_BANDPASS, FDSP_SVF_NOTCH, FDSP_SVF_PEAK,
       FDSP_SVF_ALLPASS, FDSP_SVF_BELL, FDSP_SVF_LOWSHELF, FDSP_SVF_HIGHSHELF };
/* BiquadCoefs constructors (src/biquad.rs:27-116) */
enum { FDSP_BQ_BUTTER_LOWPASS = 0, FDSP_BQ_RESONATOR, FDSP_BQ_LOWPASS, FDSP_BQ_HIGHPASS, FDSP_BQ_BELL };

typedef struct fdsp_bank fdsp_bank;

const char* fdsp_last_error(void);

/* ---- voice-graph kinds compiled into the library -------------------------------------------------------
 * Leaves (each replaces that node's AudioNode::process):
 *   "sine" oscillator.rs:21  "noise" noise.rs:173  "fixed_svf" svf.rs:861  "svf3"/"svf4" svf.rs:748
 *   "biquad" biquad.rs:136  "biquad_bank" biquad_bank.rs:14 (voice = instance*8 + lane)
 *   "butterpass_hz"/"butterpass" biquad.rs:227  "resonator_hz"/"resonator" biquad.rs:310
 *   "moog_hz"/"moog" moog.rs:17  "fir2"/"fir3" fir.rs:14  "tick" delay.rs:19  "pass" audionode.rs:408
 * Fused BASELINE graphs (combinator semantics of audionode.rs Pipe/Unop/Constant are fused in registers):
 *   "sine_hz"            constant(f) >> sine()                                         prelude.rs:349
 *   "sine_hz_lowpass_hz" sine_hz(f) >> lowpass_hz(fc, q)                    (BASELINE config 1)
 *   "noise_biquad"       noise() >> biquad(..)        one BiquadBank lane  (BASELINE config 2)
 *   "fm_svf"             sine_hz(f) * f * m + f >> sine() >> lowpass_hz(fc, q) (BASELINE config 3)
 *   "saw_moog_adsr_pan"  ((dc(f) >> saw() | dc(fc) | dc(q)) >> moog()) * adsr_live(a,d,s,r) >> pan(p)
 *                        1 input (gate), 2 outputs                            (BASELINE config 4 voice)
 * Delay lines (need fdsp_bank_create_ring): "delay" delay.rs:72, "tap" :148, "tap_linear" :386,
 *   "allnest_delay"/"allnest_tick"/"allnest_pass" :294 (AllNest around Delay / Tick / Pass)
 * Shapers and oscillators: "shape" shape.rs:205 (per-voice shape kind), "ramp"/"poly_saw"/"poly_square"/"poly_pulse"
 *   oscillator.rs:441-760, "rossler"/"lorenz" :323-435; nonlinear biquads "fbiquad_hz"/"dbiquad_hz"/"fbiquad3"/
 *   "fbiquad4"/"dbiquad3"/"dbiquad4" biquad.rs:494-920
 * More leaves: "saw"/"square"/"triangle" wavetable.rs:249 (need fdsp_wavetable_build/upload first),
 *   "adsr_live" adsr.rs:21 + envelope.rs:185, "pan" pan.rs:26
 */
int fdsp_kind_count(void);
const char* fdsp_kind_name(int kind);
int fdsp_kind_by_name(const char* name); /* -1 if unknown */
/* Engine options.  "pipe_split" (default 1): render Pipe-chain graphs of the ahead-of-time kinds in the voice-minor
 * layout with the multi-wave pipeline split (the chain stages of each 64-voice group cut into 2 or 3 consecutive
 * segments that run in 2 or 3 waves sharing a SIMD; identical samples, better issue-slot utilisation at one
 * voice-wave per SIMD).  1 = best plan, 2 / 3 = exactly that many stages (if the graph allows), 0 = single-wave kernel.
 * With 1 the launch length decides as well: a chain worth cutting takes the pipeline from ONE 64-frame block on (a light graph such
 * as noise >> biquad from four blocks on, planar launches from 16 frames on), small banks of oscillator chains the time-split kernels
 * from one whole block on, anything shorter the single-wave kernel; 2 / 3 force the pipeline at any length.  Same samples always. */
int fdsp_set_option(const char* name, int value);
/* "math" (default FDSP_MATH_EXACT): the arithmetic of banks created afterwards.
 *   FDSP_MATH_EXACT  every node evaluates the reference's own algorithm operation for operation (no contraction, the
 *                    restated libm / wide functions): bit-identical to the CPU oracle.  The headline mode.
 *   FDSP_MATH_FAST   tolerance mode: state recurrences (phases, filter states, envelopes) stay operation for operation,
 *                    but feed-forward transcendental evaluations may use the engine's own forms -- today the f32x8
 *                    sine of Sine::process (FMA polynomial, 13 instead of 28 operations, within 1.2e-7 of it) and the
 *                    saturating tanh of Moog::process (hardware exp2 / reciprocal, odd polynomial below |x| = 0.25;
 *                    within 2.3e-7 absolute / 6.3e-7 relative over all f32; the BASELINE config-4 voice within 1e-4 of the exact mode,
 *                    measured 4e-7).  Stated tolerance of the sine,
 *                    measured in tests/test_gpu_math_fast.py on the BASELINE config-3 FM voices against the exact mode:
 *                    <= 1e-4 absolute over the reference's own check window (441 samples, tests/test_basic.rs:21-47);
 *                    <= 1e-3 max, <= 5e-5 rms over a full second (measured 2.6e-4 / 1.2e-5) -- an FM patch integrates
 *                    every last-bit difference of the modulator into the carrier phase: the reference's own tick and
 *                    process paths drift ~0.2 apart over the same second.  Kinds without such a node render exactly.
 * Per bank: fdsp_bank_set_option(bank, "math", v) / fdsp_bank_get_option(bank, "math");
 * fdsp_bank_get_option(bank, "math_has_fast_variant") tells whether FAST changes anything for the bank's kind. */
#define FDSP_MATH_EXACT 0
#define FDSP_MATH_FAST 1
int fdsp_bank_set_option(fdsp_bank* bank, const char* name, int value);
int fdsp_bank_get_option(const fdsp_bank* bank, const char* name);
/* The launch options -- "pipe_split", "time_split" (default 1: banks of <= 2 voice groups per CU of eligible graphs take
 * the time-split kernel), "fdn_kernel", "timing" -- exist per bank as well: fdsp_bank_set_option(bank, name, v) overrides
 * the process-wide value of fdsp_set_option for that bank (-1 = follow it again).  They are resolved per launch on the
 * calling thread, so hosts driving different banks from different threads do not see each other's choices.
 * "timing" (default 1): every render records a HIP event pair around the kernel (fdsp_bank_last_kernel_ms); 0 drops
 * the pair -- a real-time host rendering one 64-frame block per call saves two event records per launch.
 * fdsp_bank_get_option(bank, "last_kernel") (read-only): the kernel family the most recent render launch took --
 * 1 single-wave, 2 pipeline, 3 planar pipeline, 4 time-split, 5 voice scheduler, 6 / 7 reverb lane-per-frame / -line,
 * 8 the chain of waves that renders a wide sum of generators (sumi / busi of >= 8 oscillators) on a small bank,
 * 9 the voice scheduler playing a score (fdsp_bank_set_score), 10 a score rendered with one lane per note ("score_exec"),
 * 11 time-split with the time-parallel filter stage ("svf_exec"). */
/* fdsp_bank_get_option(bank, "has_fused_mix") (read-only): 1 if fdsp_bank_process_mix has kernels for the bank's kind (voice banks), or
 * the bank is a reverb / network bank (their mix-down renders into a scratch: "the stereo mix-down" below); 0 for resynthesizer and convolver banks. */
/* "fx_mix_chunk_frames" (default 0 = automatic, from a 256 MiB budget): frames per chunk of the mix scratch of a reverb / network bank, a
 * multiple of 64 (FDSP_EINVAL otherwise).  The chunking changes no bit of the mix. */
/* "score_exec" (per bank, default FDSP_SCORE_VOICES): how fdsp_bank_process_events / _mix execute a score (fdsp_bank_set_score).
 *   FDSP_SCORE_VOICES  a lane is a VOICE and walks the launch frame by frame: the cost is voices x frames however many notes there
 *                      are.  For scores whose notes are long next to the launch (sustained voices, a real-time host's 64-frame blocks).
 *   FDSP_SCORE_NOTES   a lane is a NOTE and walks only the blocks its note lives in; the output is zeroed first and the voices' state
 *                      is committed by a small second kernel.  The cost is (longest note) x (waves of notes / chip): for long launches
 *                      over many short notes.  Same samples, same state, same clock, bit for bit.
 * A request, like "pipe_split": setting it always succeeds on a voice bank (effect banks: FDSP_EINVAL), a kind that cannot take the
 * note path keeps the voice path silently ("last_kernel" then reads 9, otherwise 10).  It is a property of the bank: setting or
 * dropping a score or events leaves it alone, fdsp_bank_clone copies it.  The bank's staging image (one copy of the slots) is allocated
 * when the option or the score is set, never in a render; a clone makes its own at its first uncaptured scored launch or in
 * fdsp_bank_mix_reserve.
 * "has_score_notes" (read-only): 1 if the bank's kind can take the note path -- a voice graph without delay rings (the notes of a voice
 * would share the ring) and without a node whose reset() keeps state (adsr_live); run-time compiled graphs answer per graph.
 * "score_chunk_frames" (default 0 = automatic, from a 256 MiB budget): fdsp_bank_process_events_mix under FDSP_SCORE_NOTES renders
 * voice-out into a scratch [outputs][chunk][voices] the bank owns and adds the voices up in the mix-down's order, chunk by chunk; this
 * is the frames per chunk, a multiple of 64 (FDSP_EINVAL otherwise).  The chunking changes no bit.  The scratch follows the partial-mix
 * buffer's rule: fdsp_bank_mix_reserve(bank, frames) sizes it, an uncaptured launch may grow it, a captured one that finds it too
 * small is refused.  "score_scratch_frames" (read-only): the frames the scratch holds now. */
#define FDSP_SCORE_VOICES 0
#define FDSP_SCORE_NOTES 1
/* "svf_exec" (launch option like "time_split": process-wide, per bank, -1 = follow the default; default FDSP_SVF_SERIAL): how the
 * time-split kernels of small banks run the fixed SVF that ends an oscillator chain.
 *   FDSP_SVF_SERIAL    one wave carries the filter's recurrence frame by frame (the reference's arithmetic; that wave is the round time).
 *   FDSP_SVF_PARALLEL  tolerance mode only: the filter is linear in its state, so every 64-frame block is rendered from state zero in
 *                      chunks of 32 frames by two waves, and a third adds what the carried state contributes (tables of the voice's
 *                      coefficients, built in f64 at the start of the launch) and carries the state on.  Not the reference's bits.
 * A request: it applies where "math" is FDSP_MATH_FAST, "time_split" is 1, the launch would take the time-split kernel (process mode,
 * voice-minor, whole blocks), the bank has at most one voice group per CU and its kind has the kernel ("has_svf_parallel", read-only:
 * 1 / 0; today fm_svf and sine_hz_lowpass_hz) -- "last_kernel" then reads 11; everywhere else the launch is exactly the one of
 * FDSP_SVF_SERIAL.  Stated tolerance, per voice, against the filter ticked in f64 on the same input:
 *   |error| <= 4.6 x (the serial f32 tick's worst error on that voice) + 2^-23 x (the voice's peak output),
 * and over a bank no worse than the serial tick's worst voice (tests/test_svf_par_host.py measures 2.3 x and the bank-wide figures;
 * tests/test_gpu_svf_par.py holds the kernel to the same bound).  Launch splits do not change a bit, the state in ic1eq / ic2eq is the
 * filter's state after the launch and either executor continues from the other's.  Non-finite samples propagate as they do serially. */
#define FDSP_SVF_SERIAL 0
#define FDSP_SVF_PARALLEL 1
/* "host_zero_copy_max" (default 262144): fdsp_bank_process_host calls moving at most this many floats per direction
 * let the kernel read/write pinned host memory directly instead of staging through HBM (lower per-block latency). */
/* "fdn_kernel" (default 0): reverb banks render with one lane per FRAME (0) or one lane per DELAY LINE (1); identical
 * samples, the former is the faster formulation. */

/* ---- run-time compiled voice graphs (graph -> kernel compiler) -------------------------------------------
 * `type_expr` is the graph's combinator TYPE, exactly what FunDSP's operators build (src/combinator.rs:289-488),
 * spelled with the engine's node templates (fundsp_amd/csrc/fd_nodes.hpp), e.g.
 *     sine_hz(f) >> lowpass_hz(fc, q)   ==  "Pipe<Pipe<Constant<1>,Sine>,FixedSvf>"
 *     (noise() | dc(fc) | dc(q)) >> moog()  ==  "Pipe<Stack<Stack<Noise,Constant<1>>,Constant<1>>,Moog<3>>"
 * The graph is compiled with hiprtc from the library's own headers (same flags as the ahead-of-time kinds) into one
 * fused kernel set and registered under `name`; fdsp_bank_create(name, ..) then works as for built-in kinds.
 * Returns the kind index (>= 0) or a negative error (fdsp_last_error() holds the compiler log).
 * fdsp_graph_check() only compiles (no device needed) -- a syntax / arity check of a type expression. */
int fdsp_graph_compile(const char* name, const char* type_expr);
/* Same, with C++ source compiled in front of the graph type (inside namespace fd): definitions the type expression
 * refers to -- typically the functor that stands in for the Rust closure of envelope(|t| ...) / lfo(|t| ...), see
 * Envelope<FN> in fundsp_amd/csrc/fd_nodes.hpp for the functor contract (OUT, visit, init, eval). */
int fdsp_graph_compile_src(const char* name, const char* type_expr, const char* source);
/* Which compiler compiles these graphs.  The promise of a run-time compiled kind -- the same samples as the same graph compiled ahead of time -- needs
 * the headers, the flags AND the compiler of the library's own build.  A host process may already hold another ROCm's libhiprtc / libamd_comgr under
 * the same sonames (a PyTorch wheel bundles ROCm 7.0's next to this image's 7.2 and loads them first); the dynamic loader then hands this library THAT
 * copy.  The library detects it and loads the libhiprtc of the ROCm it was built against into a link-map namespace of its own (dlmopen), where it finds
 * its own comgr.  Returns a description: "linked: <path>" (the process's hiprtc is the right one) or "isolated: <path> (the process's own is <path>)".
 * Environment: FDSP_HIPRTC=linked keeps the process's copy whatever it is, FDSP_HIPRTC=<path of a libhiprtc.so> names another one;
 * FDSP_JIT_DUMP=<directory> writes the generated source and code object of every compiled module there.  Why it matters: the bundled 7.0 compiler
 * miscompiles one kernel variant of `(mls() ^ impulse()) + c` (DESIGN.md section 0, round 6 "third part, 4"; tests/test_gpu_jit_compiler.py). */
const char* fdsp_jit_compiler(void);
int fdsp_graph_check(const char* type_expr);
/* The Rust side of the compiler: hand over `core::any::type_name::<X>()` of the graph `An<X>` as it is, e.g.
 *   fundsp::combinator::An<fundsp::audionode::Pipe<fundsp::audionode::Pipe<fundsp::audionode::Constant<typenum::uint::
 *   UInt<typenum::uint::UTerm, typenum::bit::B1>>, fundsp::oscillator::Sine<f32>>, fundsp::svf::FixedSvf<f32,
 *   fundsp::svf::LowpassMode<f32>>>>
 * fdsp_rust_type_to_expr rewrites it with the engine's templates ("Pipe<Pipe<Constant<1>,Sine>,FixedSvf>") and lists
 * the parameters the Rust TYPE carries as "slot=value" lines ("1:mode=0": filter modes, shape kinds, biquad modes;
 * combinator.rs:178-488, audionode.rs:850,1232,1375,1496).  fdsp_graph_compile_rust compiles the result under `name`
 * (like fdsp_graph_compile_src; `source` = functor definitions for closures, or NULL) and remembers those presets:
 * every bank created from the kind gets them applied.  Field VALUES (frequencies, Q ..) are not in a type: set them with
 * fdsp_bank_set_param as for any kind.  `hints` (or NULL) supplies what neither the type nor a slot carries, consumed
 * in the order the nodes appear in the type:
 *   "wavesynth=saw,square;meter=peak,rms;envelope=EnvExp;envelope_in=MyFn;map=MidSide;shape_fn=SoftFold" */
int fdsp_rust_type_to_expr(const char* rust_type_name, const char* hints, char* out_expr, size_t expr_cap,
                           char* out_presets, size_t presets_cap);
int fdsp_graph_compile_rust(const char* name, const char* rust_type_name, const char* hints, const char* source);
/* Host-only introspection of a kind (no device needed): arity and the named per-voice slots. */
int fdsp_kind_inputs(int kind);
int fdsp_kind_outputs(int kind);
int fdsp_kind_slot_count(int kind);
const char* fdsp_kind_slot_name(int kind, int slot);
int fdsp_kind_slot_kind(int kind, int slot);

/* ---- lifecycle (mirrors constructors / AudioNode::{set_sample_rate,reset,set_seed}) --------------------- */
/* Creates a bank of `voices` instances on the current HIP device.  State after creation equals the
 * reference constructor: DEFAULT_SR, default parameters, combinator construction-time ping (audionode.rs:871-876). */
int fdsp_bank_create(const char* kind, size_t voices, fdsp_bank** out);
/* Kinds that contain delay lines ("delay", "tap", "tap_linear", "allnest_delay": src/delay.rs) keep their rings in HBM,
 * laid out [ring node][position][voice].  `ring_frames` is the capacity (positions) of every ring of the graph and must
 * cover the longest delay at the highest sample rate that will be set: Delay needs round(time*sr)+1, Tap
 * next_pow2(ceil(max_delay*sr)+11), TapLinear next_pow2(ceil(max_delay*sr)+2) (delay.rs:108-110,204-206,440-442). */
int fdsp_bank_create_ring(const char* kind, size_t voices, size_t ring_frames, fdsp_bank** out);
/* reverb_stereo(room_size, time, damping) (src/prelude.rs:1732-1762): bank of `instances` independent 32-line FDN
 * reverbs, 2 inputs / 2 outputs each, all with the same parameters.  Default mapping: one wave per instance, one lane
 * per FRAME of a 64-sample block (the 32 lines in 32 registers, the Hadamard as register butterflies; option
 * "fdn_kernel" = 1 selects the lane-per-delay-line formulation, identical samples); delay rings in HBM; flushes f32
 * denormals like the reference does after Feedback::new (src/feedback.rs:96, src/denormal.rs:18).  The handle works
 * with set_sample_rate / reset / process / clone / destroy.  Layouts: FDSP_LAYOUT_PLANAR ([instance][channel][frame_stride]) is what a
 * lane-per-frame kernel reads and writes in 256-byte runs; FDSP_LAYOUT_VOICE_MINOR buffers of banks with 64 instances or more go
 * through a planar staging copy owned by the bank (one tiled transpose in, one out: + 8 bytes per channel and instance-frame; it grows
 * with the longest launch, outside stream captures only -- a captured launch that finds it too small gathers directly), smaller banks
 * gather them directly. */
int fdsp_reverb_stereo_create(size_t instances, double room_size, double time, double damping, fdsp_bank** out);
/* reverb4_stereo(room_size, time) (src/prelude.rs:1873-1941): TWO 16-line Hadamard networks in series --
 * multisplit::<U2,U8>() >> fdn(16 x delay >> fir3) >> multijoin::<U2,U8>() >> multisplit::<U2,U8>() >> fdn(16 x delay >> fir3)
 * >> sumf::<U16>(pan) * dc((1/4, 1/4)) -- through the same lane-per-frame kernel (both networks' ring reads, FIR outputs and feedback
 * are known at the head of a block; 272 B per instance-frame as well).  FDSP_MODE_PROCESS / FDSP_MODE_TICK differ in MultiJoin's
 * arithmetic exactly like the reference (src/audionode.rs:697-720).  Same handle semantics as reverb_stereo banks; "fdn_kernel" is ignored. */
int fdsp_reverb4_stereo_create(size_t instances, double room_size, double time, fdsp_bank** out);
/* reverb4_stereo_delays(delays, time) (src/prelude.rs:1917-1941): the same two networks with the caller's 32 delay times -- one table for
 * the bank (per_instance = 0, delays = [32]) or one per instance (per_instance = 1, delays = [instances][32]): the candidates of
 * examples/optimize.rs (src/reverb.rs:17-28), thousands of them in lock-step.  Delays are f32 seconds as the reference takes them
 * (Delay::new(delays[i] as f64)); `time` enters through a = pow(db_amp(-60), 0.03 / time) as f32 (room_size is 10 here, :1921).  The
 * lane-per-frame kernel reads the instance's 32 ring lengths from a device table; everything else -- both layouts, PROCESS / TICK,
 * set_sample_rate (every row is re-derived, the 128-sample rule checked over all of them, nothing changes on failure), reset, clone,
 * fdsp_bank_set_bus, the fused mix-down, flushed denormals -- is fdsp_reverb4_stereo_create's.  FDSP_EINVAL before anything is allocated
 * for a NULL table, a delay that is negative or not a number, or one under 128 samples at 44.1 kHz.
 * RING CAPACITY: one power of two for the bank, fixed by the longest delay given HERE or 0.070 s x 1.5 = 0.105 s, whichever is larger
 * (at the current rate; 8 192 slots at 44.1 and 48 kHz for the search range 0.030-0.070 s). */
int fdsp_reverb4_stereo_delays_create(size_t instances, const float* delays, int per_instance, double time, fdsp_bank** out);
/* Replace the delay rows of instances first .. first+count-1 ([count][32] f32 seconds, borrowed for the call; a bank with one table has
 * the single row 0) between launches, in stream order, and reset those instances (all of them where the bank shares one row): one search
 * round is one upload, not a new bank.  FDSP_EINVAL, with nothing changed, for a bank of another kind, rows out of range, a delay that
 * is negative, not a number or under 128 samples at the bank's rate, or one that needs a larger ring than the bank has. */
int fdsp_reverb4_set_delays(fdsp_bank* bank, const float* delays, size_t first, size_t count);
/* reverb_fitness (src/reverb.rs:31-139) of every instance of an effect bank with 2 inputs and 2 outputs -- the reverbs, stereo networks,
 * a two-channel convolver -- on the device: the bank is reset, renders Impulse::<U2> (1.0 on both channels at frame 0) for 32 768 frames
 * in FDSP_MODE_PROCESS at its current sample rate (the reference's number is at 44 100 Hz, the default) into scratch it owns, every
 * (instance, channel) response is scored (echo density; Hann window, real FFT, outliers above the mean of the 50 bins before), and the
 * bank is reset again: it is left as constructed.  d_fitness = [instances] device floats; d_terms, if not NULL, [instances][4] =
 * echo_0, pen_0, echo_1, pen_1 with fitness = echo_0 - pen_0 + echo_1 - pen_1.  Every sum has a fixed order (fd_fitness.hpp): the
 * same bits run to run and for any bank size.  The scratch -- 2 x instances x 2 x 32 768 floats, the render kernels take one stride for
 * input and output -- is allocated by fdsp_bank_fitness_reserve or by the first call, kept until the bank goes and not cloned
 * (fdsp_bank_get_option(bank, "fitness_scratch_kib") reads its size, 0 while there is none; "fitness_allocs" counts the device
 * allocations made for these calls so far -- 2 once reserved, for good; "fitness_score_us" is the device time of the last call's
 * scoring kernels in microseconds).
 * FDSP_ENOTSUP for voice banks and other arities; FDSP_EINVAL on a stream that is being captured. */
int fdsp_bank_fitness_reserve(fdsp_bank* bank);
int fdsp_bank_reverb_fitness(fdsp_bank* bank, float* d_fitness, float* d_terms, void* stream);
/* The generic Hadamard feedback delay network as the prelude documents it (src/prelude.rs:1323-1345, "Mono Reverb" :1334):
 *     split::<N>() >> fdn::<N, _>(stacki::<N, _, _>(|i| delay(delays[i]) >> fir(weights))) >> join::<N>()
 * `instances` independent networks of `lines` = N delay lines (2, 4, 8, 16 or 32), Delay::new(delays[i]) seconds each
 * (src/delay.rs:82-113), every line followed by the same Fir of `taps` = 1..3 weights (src/fir.rs:14-70), Feedback with FrameHadamard
 * around them (src/feedback.rs:35-57,108-146).  `inputs` = 1 puts split::<N>() in front (src/audionode.rs:527-568), 2
 * multisplit::<U2, N/2>() (:571-613: line k takes channel k % 2); `outputs` = 1 puts join::<N>() behind (:617-660), 2
 * multijoin::<U2, N/2>() (:668-730; FDSP_MODE_PROCESS scales every term by 1/n and adds, FDSP_MODE_TICK adds and divides, like the
 * reference's two executors).  Rendered by the lane-per-frame kernel of the reverbs (one wave per instance, the lines in registers, ring
 * rows as 256-byte runs: 8 * lines + 4 * (inputs + outputs) bytes per instance-frame), which needs every delay to exceed two blocks
 * (128 samples) at the bank's sample rate -- FDSP_EINVAL otherwise; such a graph still renders lane-per-voice through
 * fdsp_graph_compile.  Flushes f32 denormals like every graph with a Feedback node.  Handle semantics of the reverb banks. */
/* Feedback delay networks beyond fdsp_fdn_create's shape: a recursive filter in every line or in the feedback loop, per-line FIR weights,
 * and every parameter per line and, with per_instance = 1, per instance.  The two forms (N = lines: 2, 4, 8, 16 or 32):
 *   FDSP_FDN_IN_LINE:  split | multisplit >> fdn(stacki(|i| delay(t_i) [>> fir(w_i)] [>> F_i] [* g_i])) >> join | multijoin
 *                      -- the output and the feedback both see the filtered line (Feedback, src/feedback.rs:108-146);
 *   FDSP_FDN_IN_LOOP:  split | multisplit >> fdn2(stacki(|i| delay(t_i) [>> fir(w_i)]), stacki(|i| F_i [* g_i])) >> join | multijoin
 *                      -- the output is the line before F; the feedback is Hadamard(F(x) * g) (Feedback2, src/feedback.rs:181-330).
 * F is lowpole_hz(cutoff_i) (FDSP_FDN_FILTER_LOWPOLE, src/filter.rs:19-66) or the FixedSvf of `svf_mode` at (cutoff_i, q_i, gain_i)
 * (FDSP_FDN_FILTER_SVF, src/svf.rs:861-1031; gain is read by bell / lowshelf / highshelf only), or nothing (FDSP_FDN_FILTER_NONE, line
 * form only).  taps = 0 means the line has no Fir node; line_gain = NULL that it has no `* g`.  Arrays are [lines] (per_instance = 0) or
 * [instances][lines] (per_instance = 1); weights have `taps` entries per line, oldest tap first.  Coefficients are computed in f32 at
 * the bank's rate.  The bank is created at `sample_rate`; every delay must be at least 128 samples there (two blocks: the lane-per-frame
 * kernel's rule) -- FDSP_EINVAL otherwise, and at a later fdsp_bank_set_sample_rate.  A change of rate empties the delay lines and keeps
 * the FIR carry, the filter states and the feedback value, like the reference.  Flushes f32 denormals.  Handle semantics of the reverb
 * banks: process (both layouts, both modes), reset, clone, fdsp_bank_set_bus. */
enum { FDSP_FDN_FILTER_NONE = 0, FDSP_FDN_FILTER_LOWPOLE = 1, FDSP_FDN_FILTER_SVF = 2 };
enum { FDSP_FDN_IN_LINE = 0, FDSP_FDN_IN_LOOP = 1 };
typedef struct fdsp_fdn_network {
    int lines, inputs, outputs, taps;   /* taps 0 = no Fir node */
    int filter;                         /* FDSP_FDN_FILTER_NONE | _LOWPOLE | _SVF */
    int svf_mode;                       /* FDSP_SVF_LOWPASS .. FDSP_SVF_HIGHSHELF */
    int place;                          /* FDSP_FDN_IN_LINE (fdn) | FDSP_FDN_IN_LOOP (fdn2) */
    int per_instance;                   /* 0: arrays are [lines]; 1: [instances][lines] */
    const double* delays;               /* seconds */
    const float* weights;               /* [..][lines][taps] */
    const float *cutoff, *q, *gain;     /* filter parameters (NULL where the filter has none) */
    const float* line_gain;             /* the `* g` behind the filter, NULL = no such node */
} fdsp_fdn_network;
int fdsp_fdn_network_create(size_t instances, const fdsp_fdn_network* net, double sample_rate, fdsp_bank** out);
/* Feedback delay banks: the identity-frame feedback around one or two delay lines -- the echo `feedback(delay(1.0) * db_amp(-3.0))`, the
 * ping-pong `feedback((delay(1.0) | delay(1.0)) >> reverse() * db_amp(-6.0))` and the combs with a filter in the loop.  `instances`
 * independent networks of `channels` = N = 1 or 2, inputs = outputs = N.  The grammar of the feedback body:
 *   FDSP_FDN_IN_LINE:  feedback( L [>> reverse()] [* g] )        (Feedback<N, X, FrameId>, src/feedback.rs:108-146)
 *   FDSP_FDN_IN_LOOP:  feedback2( L [>> reverse()], Y )          (Feedback2<N, X, Y, FrameId>, src/feedback.rs:233-276)
 *     L      = line  |  line_0 | line_1
 *     line_i = delay(t_i) [>> fir(w_i..)] [>> F_i] [* g_i]       (loop form: delay [>> fir] only)
 *     Y      = F [* g]  |  (F_0 [* g_0]) | (F_1 [* g_1])
 *     F      = lowpole_hz(c) (FDSP_FDN_FILTER_LOWPOLE) | the FixedSvf of `svf_mode` at (cutoff, q, gain) (FDSP_FDN_FILTER_SVF) | nothing
 *              (FDSP_FDN_FILTER_NONE, line form only)
 * taps = 0 means the line has no Fir node (1..3 otherwise, oldest tap first); line_gain = NULL that it has no `* g_i`; outer_gain = NULL that
 * the body has no `* g` (line form only); reverse != 0 puts reverse() behind the two lines (N = 2 only).  Arrays are [channels]
 * (per_instance = 0) or [instances][channels] (per_instance = 1); outer_gain is [1] or [instances].
 * Per frame n and channel c, all in f32, one rounding per operation, subnormals flushed (Feedback::new calls prevent_denormals), in this order:
 *   1. xin_c = in_c[n] + value_c;   2. d_c = Delay::tick(xin_c), len = round(t * sample_rate) + 1;
 *   3. o_c = Fir::tick if taps, then F if it is in the line, then * g_c if the line has a gain;
 *   4. p_c = o_perm(c) (identity or reversal), then p_c * g if the body has the outer gain;
 *   5. line form: output_c = value_c = p_c (FrameId::frame multiplies by nothing);
 *   6. loop form: output_c = p_c, value_c = F_c(p_c) [* g_c].
 * FDSP_MODE_TICK and FDSP_MODE_PROCESS give the same bits, and so does every split of an input into launches.
 * Rules: every delay must be at least 128 samples at the bank's rate (two blocks: the lane-per-frame kernel's rule) and no ring may exceed
 * 2^18 slots -- FDSP_EINVAL otherwise, at creation and at a later fdsp_bank_set_sample_rate (which then changes nothing).  A change of rate
 * empties the delay lines and keeps the FIR carry, the filter states and the feedback value, like the reference.  Handle semantics of the
 * reverb banks: process (both layouts), reset, clone, fdsp_bank_set_bus, the fused mix-down (FDSP_MIX_SUM; FDSP_MIX_PAN for N = 1). */
typedef struct fdsp_feedback_delay {
    int channels, taps;                 /* N = 1 | 2; taps 0 = no Fir node */
    int filter;                         /* FDSP_FDN_FILTER_NONE | _LOWPOLE | _SVF */
    int svf_mode;                       /* FDSP_SVF_LOWPASS .. FDSP_SVF_HIGHSHELF */
    int place;                          /* FDSP_FDN_IN_LINE (feedback) | FDSP_FDN_IN_LOOP (feedback2) */
    int reverse;                        /* 1: reverse() behind the lines (N = 2) */
    int per_instance;                   /* 0: arrays are [channels]; 1: [instances][channels] */
    const double* delays;               /* seconds */
    const float* weights;               /* [..][channels][taps] */
    const float *cutoff, *q, *gain;     /* filter parameters (NULL where the filter has none) */
    const float* line_gain;             /* the `* g_i` behind the line / the loop filter, NULL = no such node */
    const float* outer_gain;            /* the `* g` behind the body: [1] | [instances], NULL = no such node */
} fdsp_feedback_delay;
int fdsp_feedback_delay_create(size_t instances, const fdsp_feedback_delay* net, double sample_rate, fdsp_bank** out);
/* Resynthesizer banks: `instances` independent resynth::<I, O, _>(window_length, processor) nodes (src/resynth.rs:216-372, prelude
 * src/prelude.rs:2825-2856) with one of three stock processing closures (o and i in increasing order, bins i = 0 .. window_length/2):
 *   FDSP_RESYNTH_PASS  fft.set(o, i, fft.at(source[o], i))                    -- FftWindow::forward, the reference's criterion bench
 *   FDSP_RESYNTH_BAND  the same where lo_hz[o] <= fft.frequency(i) <= hi_hz[o] -- the prelude's brickwall example
 *   FDSP_RESYNTH_GAIN  fft.set(o, i, fft.at(source[o], i) * gain[o][i])        -- Complex32 times f32
 * source[o] = -1 leaves output o silent.  window_length N is a power of two from 4 to 8192; inputs and outputs take 1 .. 8.  Tables are
 * [outputs] (per_instance = 0) or [instances][outputs] (per_instance = 1); gain has N/2 + 1 entries per output.  flush_denormals = 1 selects the
 * flush-to-zero build of the kernels: the reference renders the whole graph flushed when a Feedback node was constructed in front of it
 * (src/denormal.rs); 0 keeps IEEE denormals like a graph without one.
 * The frames that complete inside a launch are independent given its input: one workgroup unit per (frame, instance, output) does the
 * source channel's real FFT and the output's inverse in LDS (64 KiB at N = 8192), the real outputs go to a frame ring in HBM, and a second
 * pass adds the four overlapping windows in the reference's window order.  Parity: bit-exact against the project's restatement of microfft's
 * rfft_N / inverse FFT (fundsp_amd/csrc/fd_resynth.hpp; microfft's own butterflies are not pinned: its source is not in the reference tree).
 * Latency N samples; a pass-through returns the input delayed by N from sample 2N on.  No process override (FDSP_MODE_PROCESS ==
 * FDSP_MODE_TICK).  set_sample_rate moves frequency() only and keeps every state; reset starts the four windows over; clone continues
 * where the source stands.  Every buffer a launch uses is allocated at creation (the frame ring takes max(256 MiB, 8 x instances x
 * outputs x N x 4 bytes)), so a launch may be captured on a caller's stream and replayed: the sample counter, the bin spacing of
 * frequency() and the tables live on the device, so a replay moves on and follows set_sample_rate / set_band / set_gain.
 * fdsp_bank_set_bus, fdsp_bank_process_mix, slots, rings and events answer FDSP_ENOTSUP; invalid specs FDSP_EINVAL before anything is
 * allocated or launched. */
enum { FDSP_RESYNTH_PASS = 0, FDSP_RESYNTH_BAND = 1, FDSP_RESYNTH_GAIN = 2 };
typedef struct fdsp_resynth_spec {
    int window_length, inputs, outputs;
    int processor;                      /* FDSP_RESYNTH_PASS | _BAND | _GAIN */
    int source[8];                      /* input channel of each output, -1 = silent */
    int per_instance;                   /* 0: tables [outputs]; 1: [instances][outputs] */
    int flush_denormals;                /* 1: f32 denormals flushed (a Feedback node in front) */
    const float *lo_hz, *hi_hz;         /* FDSP_RESYNTH_BAND: [..][outputs] */
    const float* gain;                  /* FDSP_RESYNTH_GAIN: [..][outputs][window_length / 2 + 1] */
} fdsp_resynth_spec;
int fdsp_resynth_create(size_t instances, const fdsp_resynth_spec* spec, fdsp_bank** out);
int fdsp_resynth_create_on(int device, size_t instances, const fdsp_resynth_spec* spec, fdsp_bank** out);
/* Replace table rows first .. first+count-1 between launches (rows are instances with per_instance, else the single row 0), with the
 * ordering of fdsp_bank_set_param: the new values apply from the next launch; the host array is borrowed for the call only.
 * set_band takes [count][outputs][2] (lo, hi) in Hz, set_gain [count][outputs][window_length / 2 + 1]. */
int fdsp_resynth_set_band(fdsp_bank* bank, const float* h_lo_hi, size_t first, size_t count);
int fdsp_resynth_set_gain(fdsp_bank* bank, const float* h_gain, size_t first, size_t count);
/* Resynthesizer banks with the CALLER's processing closure: resynth::<I, O, _>(window_length, |fft| ...) where the closure is a C++ functor
 * in namespace fd, given as source text in the per-bin form and compiled by the library's own run-time compiler when the bank is created
 * (never inside a render: a first launch can be captured).  fundsp_amd/csrc/fd_resynth_fn.hpp states the contract -- bin(fft, i) is called
 * once per frame and bin, reads any input bin through fft.at(channel, j) and writes output bin i only through fft.set(channel, i, value);
 * fft mirrors FftWindow (bins, frequency, the time() family in f64, param(p), state(s)) -- and the three stock closures as functors.
 * `functor` names the type, `source` defines it; `params` f32 values per instance (0 .. 65536) and `state` f32 values per (instance, bin)
 * (0 .. 16) must equal the functor's PARAMS / STATE.  param_values is [instances][params], NULL = zeros.  With state > 0 the frames of an
 * instance are processed in increasing order.  The forward and inverse transforms are the stock bank's, cut at the spectra, which pass
 * through a workspace of instances x Fc x (inputs + outputs) x (N/2 + 1) x 8 bytes (Fc frames per chunk, chosen so that the workspace does
 * not exceed the frame ring); everything is allocated at creation.  A compile error answers FDSP_EINVAL with the compiler's log in
 * fdsp_last_error() and allocates nothing.  reset zeroes the state and restarts the windows; clone copies state and parameters;
 * set_sample_rate moves frequency() and the time() family only.  fdsp_resynth_set_band / _gain on a closure bank and
 * fdsp_resynth_set_params on a stock bank answer FDSP_ENOTSUP; bus, mix-down, slots, rings and events FDSP_ENOTSUP as for the stock banks. */
typedef struct fdsp_resynth_fn_spec {
    int window_length, inputs, outputs;
    int params;                         /* f32 parameters per instance: the functor's PARAMS */
    int state;                          /* f32 state values per (instance, bin): the functor's STATE */
    int flush_denormals;                /* 1: f32 denormals flushed (a Feedback node in front) */
    const char* functor;                /* the type's name in namespace fd */
    const char* source;                 /* its definition */
    const float* param_values;          /* [instances][params], NULL = zeros */
} fdsp_resynth_fn_spec;
int fdsp_resynth_fn_create(size_t instances, const fdsp_resynth_fn_spec* spec, fdsp_bank** out);
int fdsp_resynth_fn_create_on(int device, size_t instances, const fdsp_resynth_fn_spec* spec, fdsp_bank** out);
/* Host only, no device (like fdsp_graph_check): checks the spec and compiles the functor's module; FDSP_EINVAL + the compiler's log. */
int fdsp_resynth_fn_check(const fdsp_resynth_fn_spec* spec);
/* Replace the parameters of instances first .. first+count-1 between launches from h_values [count][params], with the ordering of
 * fdsp_bank_set_param: they apply from the next launch, i.e. to the frames completing at sample counts above the launch's start. */
int fdsp_resynth_set_params(fdsp_bank* bank, const float* h_values, size_t first, size_t count);
/* Host only, no device: the bank's tables for window_length N -- hann[N] = 0.5 + 0.5 * cosf(((i - N/2) as f32 * TAU) / N as f32) and
 * twiddles[N/2][2] = (cos, -sin)(2 pi j / N) computed in double and rounded to f32.  Either pointer may be NULL. */
int fdsp_resynth_tables(int window_length, float* h_hann, float* h_twiddles);
/* Convolver banks: `instances` x `channels` independent convolve(&wave, channel) nodes (src/convolve.rs, src/prelude.rs:3154-3160; the
 * reference's stereo form is convolve(&w, 0) | convolve(&w, 1)): channel c is its own 1 -> 1 convolver with response row c,
 *   y[n] = sum over k < len of h[k] * x[n - k],  x[n < 0] = 0,  no latency,
 * in f32 by uniformly partitioned FFT convolution that this project states operation by operation in fundsp_amd/csrc/fd_convolve.hpp:
 * block length B chosen from the capacity max_len (fdsp_convolve_block_length), one forward transform per COMPLETE block, the partitions'
 * products summed in increasing partition order, one inverse per block for the part of the output that older blocks decide, and the
 * current block's own samples added directly (h[0] * x[n] first, then h[i] * x[n - i] for increasing i).  Only complete blocks are ever
 * transformed, so every split of an input into launches -- one launch, sample by sample, ragged, a captured launch replayed -- gives the
 * same bits, and FDSP_MODE_PROCESS == FDSP_MODE_TICK.  Parity: bit-exact against that statement (tests/convolve_ref.py restates it in
 * numpy), and that statement within 4.1e-7 of a float64 convolution at B = 64 (capacities up to 512 taps) and within 9.5e-7 at B = 128 ..
 * 4096, relative to sum |h| x max |x| (tests/test_convolve_ref.py; the largest figures belong to short responses under a large capacity).
 * The reference wraps the crate fft_convolver, whose source is not in the reference tree: the crate's own bits (its butterflies,
 * its partition scheme, any trimming of trailing near-zero taps) are NOT pinned; what the reference's tests ask -- no latency, the known
 * answer and tick == process within 1e-4 -- holds.
 * response is [rows][channels][len], rows = instances with per_instance = 1, else 1.  max_len is the capacity: nothing is allocated,
 * grown or freed after creation, so a launch may be captured on a caller's stream and replayed (the sample counter and the lengths live
 * on the device: a replay moves on and follows set_response).  With Pcap = ceil(max_len / B) and KB = clamp(256 MiB / (instances x
 * channels x (B + 1) x 8 B), 8, 64) a bank takes
 *   instances x channels x (Rx x 4 + (Pcap + 2 KB) x (B + 1) x 8 + (KB + 1) x B x 4) + rows x channels x ((Pcap + 1) x B x 4 + Pcap x (B + 1) x 8)
 * bytes, Rx the power of two at or above (KB + 1) x B.  flush_denormals = 1 selects the flush-to-zero build (a Feedback node in front, as
 * for the resynthesizer).  set_sample_rate is accepted and changes nothing (the node has no override); reset clears the history; clone
 * continues where the source stands.  fdsp_bank_set_bus, fdsp_bank_process_mix, slots, rings and events answer FDSP_ENOTSUP; invalid specs
 * FDSP_EINVAL before anything is allocated or launched. */
typedef struct fdsp_convolve_spec {
    int channels;                       /* 1 .. 8 */
    size_t max_len;                     /* response capacity in taps, 1 .. 2^24 */
    size_t len;                         /* 1 .. max_len */
    int per_instance;                   /* 0: response [channels][len]; 1: [instances][channels][len] */
    int flush_denormals;                /* 1: f32 denormals flushed (a Feedback node in front) */
    const float* response;
} fdsp_convolve_spec;
int fdsp_convolve_create(size_t instances, const fdsp_convolve_spec* spec, fdsp_bank** out);
int fdsp_convolve_create_on(int device, size_t instances, const fdsp_convolve_spec* spec, fdsp_bank** out);
/* Routed convolver banks: ONE input through SEVERAL responses, the reference's Branch of convolvers -- a mono voice into a stereo room is
 * convolve(&w, 0) ^ convolve(&w, 1), a stereo source into a four-channel response (ll ^ lr) | (rl ^ rr).  The bank has `inputs` inputs and
 * spec->channels outputs, 1 <= inputs <= channels <= 8; output c is the 1 -> 1 convolver of the contract above with response row c,
 * reading input source[c] (source holds `channels` entries in [0, inputs), borrowed for the call; every input feeds at least one output).
 * No operation and no order changes: the bits are those of fdsp_convolve_create fed copies of the input rows, and the identity map gives
 * the plain constructor's bits.  What is shared is the input side -- the input ring, the forward transform of every block and the
 * spectrum ring (the frequency-domain delay line) exist once per (instance, INPUT); the response tables, the partition sums, the inverse
 * transform, the pending ring and the direct head stay per (instance, OUTPUT), and outputs of one input are rendered two at a time from
 * one load of each block spectrum and of each input sample (fd_convolve.hpp "fan groups").  KB keeps its formula with channels = outputs,
 * so the chunks are the plain bank's, and a bank takes
 *   instances x (inputs x (Rx x 4 + (Pcap + KB) x (B + 1) x 8) + channels x (KB x (B + 1) x 8 + (KB + 1) x B x 4))
 *     + rows x channels x ((Pcap + 1) x B x 4 + Pcap x (B + 1) x 8)
 * bytes.  response, fdsp_convolve_set_response (rows [channels][len], channels = outputs), reset, clone, set_sample_rate, capture and
 * the FDSP_ENOTSUP answers are those of fdsp_convolve_create.  FDSP_EINVAL with a message that names the field, before anything is
 * allocated or a device is touched: what fdsp_convolve_create refuses, inputs < 1 or inputs > channels, source NULL, an entry outside
 * [0, inputs), an input that feeds no output. */
int fdsp_convolve_routed_create(size_t instances, const fdsp_convolve_spec* spec, int inputs, const int* source, fdsp_bank** out);
int fdsp_convolve_routed_create_on(int device, size_t instances, const fdsp_convolve_spec* spec, int inputs, const int* source, fdsp_bank** out);
/* Summing convolver banks: SEVERAL inputs convolved and ADDED into one output, the reference's Binop<FrameAdd> over convolvers
 * (src/audionode.rs:903-955) -- convolve(&w, 0) + convolve(&w, 1); a true-stereo impulse response is (ll + rl) ^ (lr + rr), 2 inputs, 4
 * responses, 2 outputs.  The bank has `inputs` inputs, `outputs` outputs and spec->channels TERMS (1 .. 16 here; inputs and outputs 1 .. 8):
 * term t convolves input term_input[t] with response row t and belongs to output term_output[t].  term_output is non-decreasing, every
 * output has at least one term, every input feeds at least one term; both tables hold `channels` entries and are borrowed for the call.
 * response is [rows][channels][len] and fdsp_convolve_set_response takes rows [channels][len], channels = terms.
 * The sum is taken in the frequency domain: the partition products of ALL terms of an output run into one sum (terms in increasing t,
 * partitions in increasing p inside a term), so one inverse transform, one pending ring and one output row serve all its terms, and the
 * direct head is one running sum over the terms too (fundsp_amd/csrc/fd_convolve.hpp states both; tests/convolve_matrix_ref.py restates
 * them in numpy and the kernels give those bits for every split into launches, FDSP_MODE_PROCESS == FDSP_MODE_TICK).  An output of ONE
 * term has exactly the routed bank's bits.  The reference adds the two nodes' rounded outputs, this bank adds before the inverse
 * transform, and the association of a `+` tree is flattened to term order: both lie inside the same float64 bound, max |y - y64| /
 * (sum over the output's terms of sum |h_t| x max |x|) <= 6.6e-7 at B = 64 and <= 9.5e-7 at B = 1024 for 1, 2, 4 and 8 terms per output
 * (tests/test_convolve_matrix_ref.py: four times the largest figure of 8 seeds; relative to that scale the error falls as terms are
 * added).  The fft_convolver crate's bits are not pinned either way.
 * KB keeps its formula with channels = outputs, and with I = inputs, O = outputs, NT = terms, V = instances, R = Pcap + KB a bank takes
 *   V x (I x (Rx x 4 + R x (B+1) x 8) + O x (KB x (B+1) x 8 + (KB+1) x B x 4)) + rows x NT x ((Pcap+1) x B x 4 + Pcap x (B+1) x 8)
 * bytes.  reset, clone, set_sample_rate, capture and replay, the FDSP_ENOTSUP answers for bus, mix-down, pan, rings and events (the bank
 * has no named slots: a slot setter answers FDSP_EINVAL, unknown slot) and the rule that nothing is allocated after creation are those of
 * fdsp_convolve_create.  FDSP_EINVAL with a message that names the field, before
 * anything is allocated or a device is touched: what fdsp_convolve_create refuses (channels beyond 16 here), inputs or outputs outside
 * 1 .. 8, a NULL table, an entry outside its range, a decreasing term_output, an output without a term, an input that feeds no term. */
int fdsp_convolve_matrix_create(size_t instances, const fdsp_convolve_spec* spec, int inputs, int outputs, const int* term_input,
                                const int* term_output, fdsp_bank** out);
int fdsp_convolve_matrix_create_on(int device, size_t instances, const fdsp_convolve_spec* spec, int inputs, int outputs, const int* term_input,
                                   const int* term_output, fdsp_bank** out);
/* Re-initialise the convolvers between launches, as Convolver::set_response does: rows first .. first+count-1 take h_response
 * [count][channels][len] (borrowed for the call), their partitions are transformed on the device, and the history of the WHOLE bank is
 * cleared (the instances share one sample counter).  len takes 1 .. max_len; a bank has one response length, so replacing only some of
 * the rows of a per-instance bank takes the current len. */
int fdsp_convolve_set_response(fdsp_bank* bank, const float* h_response, size_t len, size_t first, size_t count);
/* Host only, no device: the block length B of a bank of capacity max_len -- the power of two at or above sqrt(8 x max_len), 64 .. 4096. */
int fdsp_convolve_block_length(size_t max_len);
/* reverb3_stereo(time, diffusion, lowpole_hz(cutoff)) (src/prelude.rs:1858-1871): the allpass-loop reverb Reverb<F> of src/reverb.rs:152-279
 * with the documented loop filter, a one-pole lowpass (src/filter.rs:19-66).  `instances` independent reverbs, 2 inputs / 2 outputs each, all
 * with the same parameters.  One wave per instance, one lane per FRAME of a 64-sample block: all 76 delay lines of the structure (4 input
 * diffusers, 8 x (4 + 4) Schroeder allpasses, 8 block delays) are longer than two blocks, so their reads are known at the head of a block and
 * every allpass is feed-forward inside it; the sixteen loop filters -- the only recurrences in time -- run on eight lanes between the two
 * allpass layers.  624 B per instance-frame (76 ring reads + 76 ring writes + 2 in + 2 out).  The graph the run-time compiler builds for the
 * same node renders the same samples one lane per voice, two to three orders of magnitude slower.  Like the reference: no process
 * override (FDSP_MODE_PROCESS == FDSP_MODE_TICK), IEEE denormals kept (no Feedback node), reset() and set_sample_rate() leave the input
 * diffusers alone (src/reverb.rs:211-238), a change of rate empties the lines but keeps every allpass's pending sample, the feedback sample
 * and the filters' values.  Needs >= 14.2 kHz (every delay longer than 128 samples).  Handle semantics and layouts of the reverb banks. */
int fdsp_reverb3_stereo_create(size_t instances, double time, double diffusion, float lowpole_cutoff_hz, fdsp_bank** out);
/* The same reverb with a FixedSvf as the loop filter -- reverb3_stereo(time, diffusion, highshelf_hz(5000.0, 1.0, db_amp(-1.0))) is what the
 * reference's examples put there (examples/keys.rs:134): svf_mode = FDSP_SVF_LOWPASS .. FDSP_SVF_HIGHSHELF (the modes of fdsp_svf_coefs),
 * `gain` an amplitude (bell / shelves).  Same kernel; the sixteen filters' recurrences (src/svf.rs:995-1006) run on the eight serial lanes. */
int fdsp_reverb3_stereo_svf_create(size_t instances, double time, double diffusion, int svf_mode, float cutoff_hz, float q, float gain, fdsp_bank** out);
int fdsp_fdn_create(size_t instances, int lines, const double* delays, int taps, const float* weights, int inputs, int outputs, fdsp_bank** out);
/* A gain and a dry bus around a reverb / network bank -- the shape the reference's documentation gives its reverbs:
 *     multipass() & 0.2 * reverb_stereo(20.0, 2.0, 1.0)                       README.md:436 ("to add 20% reverb to a stereo signal")
 *     0.2 * reverb_stereo(10.0, 1.0, 0.5) & multipass()                       src/wave.rs:514
 *     wet * reverb_stereo(10.0, time) & (1.0 - wet) * multipass()             CHANGES.md:203
 * `wet * node` is Unop<X, FrameMulScalar> (src/combinator.rs:477-488, src/audionode.rs:1190-1228: every output sample times the scalar),
 * `x & y` is Bus<X, Y> (src/audionode.rs:1842-1877: both sides take the node's input and the outputs are added, one addition per sample in
 * tick :1862-1866 and in process :1868-1877), multipass() hands its input on (:373-403).  The render kernels fold these nodes into their
 * epilogue (the block's input frames are still in registers there; no second pass over the output, no buffer for the wet signal):
 *     FDSP_BUS_NONE     out = node(in)                          (the bank as created)
 *     FDSP_BUS_WET      out = wet * node(in)                    `wet * node`; `dry` ignored
 *     FDSP_BUS_DRY_WET  out = dry * in + wet * node(in)         `dry * multipass() & wet * node` in either order of the `&` (f32 addition commutes);
 *                                                               needs inputs == outputs (Bus: both sides have the same arities)
 * one f32 rounding per multiplication and per addition, as the reference's three nodes; pass 1.0 for a factor the graph does not have (x * 1.0 is x
 * bit for bit, so `multipass() & 0.2 * node` is (FDSP_BUS_DRY_WET, 0.2, 1.0) and `multipass() & node` (src/net.rs:681) is (.., 1.0, 1.0)).  A host-side
 * setting: takes effect at the next launch, survives reset / set_sample_rate, travels with fdsp_bank_clone.  Banks of the reverb / network
 * constructors above only (FDSP_ENOTSUP otherwise: a compiled graph carries its bus in its type).  The nodes' pings are no concern of the bank: none
 * of these nodes keeps hashed state (a generator in FRONT of the bus is seeded by the host from the whole graph's construction hash). */
#define FDSP_BUS_NONE 0
#define FDSP_BUS_WET 1
#define FDSP_BUS_DRY_WET 2
int fdsp_bank_set_bus(fdsp_bank* bank, int mode, float wet, float dry);
int fdsp_bank_get_bus(const fdsp_bank* bank, int* mode, float* wet, float* dry);
/* Several GPUs from one process.  A bank lives on ONE device, fixed at creation: the `_on` constructors take the HIP
 * device index (-1 = the calling thread's current device, which is what the constructors above use).  Every entry point
 * that takes a bank makes the bank's device current for its own duration and restores the caller's, so a host thread
 * may interleave banks of different GPUs freely; a bank is still single-threaded (AudioNode::process(&mut self)),
 * different banks may be driven from different threads.  Shared wavetables / waves are kept per device and installed
 * on every device that has banks.  `ring_frames` = 0 for kinds without delay lines. */
int fdsp_device_count(void);
int fdsp_bank_create_on(int device, const char* kind, size_t voices, size_t ring_frames, fdsp_bank** out);
int fdsp_reverb_stereo_create_on(int device, size_t instances, double room_size, double time, double damping, fdsp_bank** out);
int fdsp_reverb4_stereo_create_on(int device, size_t instances, double room_size, double time, fdsp_bank** out);
int fdsp_reverb4_stereo_delays_create_on(int device, size_t instances, const float* delays, int per_instance, double time, fdsp_bank** out);
int fdsp_reverb3_stereo_create_on(int device, size_t instances, double time, double diffusion, float lowpole_cutoff_hz, fdsp_bank** out);
int fdsp_reverb3_stereo_svf_create_on(int device, size_t instances, double time, double diffusion, int svf_mode, float cutoff_hz, float q, float gain, fdsp_bank** out);
int fdsp_fdn_create_on(int device, size_t instances, int lines, const double* delays, int taps, const float* weights, int inputs, int outputs, fdsp_bank** out);
int fdsp_fdn_network_create_on(int device, size_t instances, const fdsp_fdn_network* net, double sample_rate, fdsp_bank** out);
int fdsp_feedback_delay_create_on(int device, size_t instances, const fdsp_feedback_delay* net, double sample_rate, fdsp_bank** out);
int fdsp_bank_device(const fdsp_bank* bank);
void fdsp_bank_destroy(fdsp_bank* bank);
/* `Clone` (every AudioNode is Clone, src/audionode.rs:35; Net and Sequencer clone their units): a new bank of the same
 * kind on the same device that continues exactly where `bank` stands -- all slots (parameters, coefficients, state), the
 * delay rings, the sample rate, the arithmetic mode and launch options, the scheduler's events and clock, a reverb's
 * line state.  Rendering the clone and the original with the same input gives the same samples. */
int fdsp_bank_clone(const fdsp_bank* bank, fdsp_bank** out);
int fdsp_bank_inputs(const fdsp_bank* bank);   /* AudioNode::Inputs  */
int fdsp_bank_outputs(const fdsp_bank* bank);  /* AudioNode::Outputs */
size_t fdsp_bank_voices(const fdsp_bank* bank);
int fdsp_bank_set_sample_rate(fdsp_bank* bank, double sample_rate); /* audionode.rs:68 */
int fdsp_bank_reset(fdsp_bank* bank);                               /* audionode.rs:52 */
/* AudioNode::set_seed (audionode.rs:366-368) per voice: ping(false, AttoHash::new(seed[i])) for voices
 * first..first+count.  h_seeds == NULL re-applies the construction-time hash to that range. */
int fdsp_bank_set_seed(fdsp_bank* bank, const uint64_t* h_seeds, size_t first, size_t count);

/* ---- parameters (mirrors AudioNode::set(Setting), setting.rs:14-72) ------------------------------------
 * Every per-voice field of the graph is a named slot "<path>:<field>[index]": <path> = child indices from the
 * root joined by '.', e.g. in "fm_svf" the filter cutoff is "1:cutoff" and the modulator frequency constant
 * is "0.0.0.0.0.0:value".  Setting a parameter re-derives dependent coefficients immediately, like the
 * reference's setters (e.g. FixedSvf::set_cutoff_q svf.rs:944-948). */
int fdsp_bank_slot_count(const fdsp_bank* bank);
const char* fdsp_bank_slot_name(const fdsp_bank* bank, int slot);
int fdsp_bank_slot_kind(const fdsp_bank* bank, int slot); /* 0 = parameter, 1 = derived coefficient, 2 = state */
int fdsp_bank_set_param(fdsp_bank* bank, const char* name, const float* h_values, size_t first, size_t count);
/* One value for every voice (Shared::set_value of a variable all voices watch, src/shared.rs:98-101): filled ON THE DEVICE in stream order behind
 * the last render -- no host copy, no host wait.  A render on the bank's own stream simply follows it; a render on a caller's stream waits for
 * it on the host as for every setter; a caller's stream that is being CAPTURED cannot wait, so a capture started while such a fill is still
 * queued is refused (FDSP_EDEVICE): call fdsp_bank_synchronize(bank) before capturing. */
int fdsp_bank_set_param_all(fdsp_bank* bank, const char* name, float value);
int fdsp_bank_set_param_u64(fdsp_bank* bank, const char* name, const uint64_t* h_values, size_t first, size_t count);
int fdsp_bank_get_slot(fdsp_bank* bank, const char* name, float* h_values, size_t first, size_t count);
/* Full per-voice snapshot, [slot_count][voices] f32 words (FunDSP nodes are Clone: audionode.rs:29). */
int fdsp_bank_get_state(fdsp_bank* bank, float* h_slots);
int fdsp_bank_set_state(fdsp_bank* bank, const float* h_slots);

/* ---- the hot path --------------------------------------------------------------------------------------
 * Render `frames` samples of every voice.  d_in may be NULL for generators.  `frame_stride` is only used by
 * FDSP_LAYOUT_PLANAR (row length in samples, >= frames; 64 for BufferArray blocks).  `stream` is a
 * hipStream_t (NULL = the bank's own stream); the call is asynchronous with respect to the host.
 * Ordering: a render on a caller's stream starts after the bank's pending parameter / lifecycle work, and later
 * setters, reset, set_seed, get/set_state wait for that render (its completion event) -- in either direction nothing
 * overtakes.  A caller's stream that is being CAPTURED into a HIP graph is supported: the launch is recorded without
 * any host-side synchronisation or event, so a real-time host can capture its block-by-block loop once and replay it
 * (tests/test_gpu_streams.py; 65 536 voices x 64 frames: 20.8 -> 13.3 us per block).  One refusal: a capture that would start behind a
 * still-queued fdsp_bank_set_param_all (the one setter that does not wait, see its comment) returns FDSP_EDEVICE and fdsp_last_error()
 * names the remedy -- fdsp_bank_synchronize(bank) before capturing.  Nothing compiles inside a render: run-time compiled kinds build
 * what a bank needs when it is created and when fdsp_bank_set_option(bank, "math", ..) switches its arithmetic.
 * Input values: every IEEE value is accepted and treated like the reference treats it (tests/test_gpu_specials.py).
 * One input sets the COST of a sample rather than its value: the speed input of Resample<X> (resample.rs:281-303) ticks
 * the enclosed generator `speed` times per output sample, on the device as in the reference -- a speed of 1e9 is a
 * billion inner ticks in one lane, i.e. a kernel that does not return in useful time.  Bound it on the host. */
int fdsp_bank_process(fdsp_bank* bank, size_t frames, const float* d_in, float* d_out, int layout,
                      size_t frame_stride, int mode, void* stream);
/* Same with host buffers (staged through device memory; synchronous).  With voices = 1, layout PLANAR,
 * frame_stride = 64 and frames = size <= 64 this is a literal AudioNode::process call on one node. */
int fdsp_bank_process_host(fdsp_bank* bank, size_t frames, const float* h_in, float* h_out, int layout,
                           size_t frame_stride, int mode);
int fdsp_bank_synchronize(fdsp_bank* bank);
/* Device time in milliseconds of the most recent fdsp_bank_process launch (HIP events on the launch stream). */
int fdsp_bank_last_kernel_ms(fdsp_bank* bank, float* ms);

/* Upload the first `frames` positions of ring node `ring_index` (visit order) for `count` voices from `first_voice`:
 * data is [count][frames] f32.  Used for state a Rust caller must provide because it comes from a crate outside the
 * reference tree: Pluck's excitation, the stream `Rnd::from_u64(hash).f32_in(-1.0, 1.0)` of funutd that
 * Pluck::initialize_line draws (src/oscillator.rs:257-261), goes into ring 0 of the "pluck" kind; Hold's draws
 * `Rnd::from_u64(hash).f64()` (src/noise.rs:299) go into that node's ring, each f64 as two f32 words, low word first. */
int fdsp_bank_set_ring(fdsp_bank* bank, int ring_index, const float* data, size_t frames, size_t first_voice,
                       size_t count);

/* ---- on-device voice scheduler: the reference's Sequencer with one event per voice (many: "scores" below) ------
 * Replaces Sequencer::push + process / tick (src/sequencer.rs:355-398, 838-951, 769-836; ReplayMode::None, no loop
 * point) for a bank whose voices are the events' units.  `events` holds 4 doubles per voice -- start_time, end_time,
 * fade_in_time, fade_out_time, seconds on the sequencer clock -- and `fade` the curve per voice (NULL = Smooth).
 * As in push(), fade times may not exceed the event's duration.  Voices without an event never play.
 * fdsp_bank_process_events renders `frames` frames from the bank's sequencer clock (0 after set_events of a fresh
 * bank; see fdsp_bank_events_rewind) into d_out [outputs][frames][voices]: each voice's own faded contribution, zeros
 * outside its event.  Their sum over voices (fdsp_sum_voices) is the Sequencer's output.  Units are processed in
 * sequencer blocks of 64 frames exactly like the reference (a unit's first and last process() block is the part of
 * the sequencer block its event overlaps), so launches other than the last should be multiples of 64 frames.
 * FDSP_MODE_TICK follows Sequencer::tick.  d_in: [inputs][frames][voices] per-voice inputs (the reference feeds
 * every event the same input; give every voice the same stream to reproduce that). */
#define FDSP_FADE_POWER 0  /* Fade::Power: equal-power crossfades (sine_ease) */
#define FDSP_FADE_SMOOTH 1 /* Fade::Smooth: equal-amplitude crossfades (smooth5), the default */
int fdsp_bank_set_events(fdsp_bank* bank, const double* events, const int* fade, size_t first_voice, size_t count);
int fdsp_bank_process_events(fdsp_bank* bank, size_t frames, const float* d_in, float* d_out, int mode, void* stream);
/* The Sequencer's OUTPUT -- the sum of its events (sequencer.rs:838-951: every active event's faded block added into the output
 * buffer) -- in one launch: d_mix [outputs][frames], the mix-down's fixed summation order (below), so it equals fdsp_sum_voices of
 * fdsp_bank_process_events' output bit for bit; the per-event samples never exist in HBM.  Graphs of at most two outputs whose kind
 * has the fused kernels (FDSP_ENOTSUP otherwise); the clock advances as in fdsp_bank_process_events. */
int fdsp_bank_process_events_mix(fdsp_bank* bank, size_t frames, const float* d_in, float* d_mix, int mode, void* stream);
/* ---- scores: many notes per voice ------------------------------------------------------------------------------
 * A pool of voices that each play one note after another, scheduled on the device, sample-exact, in one launch: the cost is
 * voices x frames however many notes the score has.  Note k has a voice index voice[k] < voices, four doubles events[4 k ..] =
 * start, end, fade_in, fade_out (seconds on the sequencer clock, the rules of Sequencer::push), a fade curve (fade == NULL:
 * FDSP_FADE_SMOOTH) and a row params[nparams k ..] of f32 values for the `nparams` (0 .. 16) per-voice f32 slots `names`.
 * The notes of one voice must not overlap (end <= next start after sorting by start; legato and several notes inside one
 * 64-frame block are fine); the input may come in any order.
 * Note k on voice v plays exactly like a Sequencer event whose unit is a FRESH unit of the bank's graph with voice v's hash
 * and voice v's parameters as they stand, the note's row written over the named slots: in the first block (tick) in which
 * the note is active the device writes the row, runs update(sample rate) and reset() -- delay rings and hashed nodes
 * included.  Everything else is the scheduler above: 64-frame blocks, the shorter first and last process() block of each
 * note, fades per block from the f64 clock, FDSP_MODE_TICK, always the exact arithmetic.
 * Where a voice stands is a function of the clock alone: its current note at clock t is the first with end > t + half a
 * sample, and a note has begun iff start < t - half a sample.  So fdsp_bank_events_rewind keeps its meaning and a note that
 * straddles a launch boundary (or a rewind) continues with the state the voice has.
 * Everything is validated before the bank is touched (FDSP_EINVAL names the offending note or slot).  The score replaces
 * any events or score of the bank; notes == 0 removes it, and so does fdsp_bank_set_events afterwards.  With a score
 * installed fdsp_bank_process_events and fdsp_bank_process_events_mix play it: output layout, clock, capture rules and the
 * fdsp_bank_mix_reserve requirement are unchanged; "last_kernel" reads 9 (10 with "score_exec" = FDSP_SCORE_NOTES, the executor for
 * long launches over many short notes: see the options above).  Run-time compiled kinds build their score kernels
 * here, never inside a render.  The slots named in the score keep the last started note's values afterwards.  Effect banks
 * answer FDSP_EINVAL; fdsp_bank_clone copies the score. */
int fdsp_bank_set_score(fdsp_bank* bank, size_t notes, const int* voice, const double* events, const int* fade, int nparams,
                        const char* const* names, const float* params);
int fdsp_bank_events_rewind(fdsp_bank* bank, double time); /* set the sequencer clock (Sequencer::reset -> 0.0) */
double fdsp_bank_events_time(const fdsp_bank* bank);       /* Sequencer::time() */

/* ---- the stereo mix-down, per GPU (SURVEY 8d "mode B", 8e "per-GPU on-device tree-sum") ------------------------------
 * What the reference computes for a bank of voices feeding one output: `voice >> pan(p)` per voice (Panner::process,
 * src/pan.rs:50-76, weights src/pan.rs:13-17), then the sum over the voices (Reduce / Net mixing, src/audionode.rs:2406-2462).
 * SUMMATION ORDER -- fixed, independent of the launch geometry, the same for every function of this section:
 *     partial(group of 64 consecutive voices) = (S0 + S1) + (S2 + S3),
 *         Sq = ((x[16q] + x[16q+1]) + x[16q+2]) + ... + x[16q+15]     (voices past the end of the bank count as +0.0)
 *     mix = the groups' partials added in an aligned binary tree: level by level node(2k) + node(2k+1), a node without a
 *         right sibling passes through unchanged.
 * So a fused mix equals fdsp_sum_voices / fdsp_mix_stereo of the voice-out render bit for bit, and both are within
 * sqrt(voices) * 6e-8 * max|x| of a serial mix (tests/test_gpu_mix.py).
 *
 * fdsp_bank_process_mix: render `frames` samples of every voice AND reduce them over the voices in the same launch -- the
 * per-voice output never exists in HBM (a voice group's last stage parks MC frames in LDS, transposes and writes one float per
 * channel and frame; a second, tiny launch adds the groups' partials).  d_in: voice-minor [inputs][frames][voices] or NULL.
 *   mix = FDSP_MIX_SUM: d_mix [outputs][frames] = sum over the voices of every output channel (graphs that end in a Panner:
 *         BASELINE config 4; the Sequencer's mix of its events);
 *   mix = FDSP_MIX_PAN: mono graphs; every voice is panned with its own position (fdsp_bank_set_pan, -1 .. 1, default 0 =
 *         centre) exactly like Panner::tick does (`weight * sample`), d_mix = [2][frames].
 * The bank owns the partial-mix buffer ([voice groups][channels][frames] f32, 1/64 of a voice-out render); it grows on demand,
 * fdsp_bank_mix_reserve(bank, frames) sizes it ahead of a real-time loop or a stream capture (AudioNode::allocate semantics).
 * A mix launch always takes the stage pipeline (or, for small banks of eligible graphs, the time-split kernel): "pipe_split" = 0 and the
 * launch-length thresholds of fdsp_bank_process do not apply to it, and a kind whose graph has no pipeline plan answers FDSP_ENOTSUP.
 * Stream, ordering, timing and capture rules are those of fdsp_bank_process (including the refusal of a capture behind a queued
 * fdsp_bank_set_param_all; run-time compiled graphs build their mix kernels in fdsp_bank_mix_reserve AND in fdsp_bank_set_pan, whichever
 * the host calls before its loop); a CAPTURED launch holds the partial-mix buffer of
 * capture time, so reserve for the longest launch before capturing and do not grow the reservation while such a graph is alive.  FDSP_ENOTSUP: the kind was built without the
 * fused kernels (the BASELINE kinds fm_svf, sine_hz_lowpass_hz, saw_moog_adsr_pan, noise_biquad have them) -- render
 * voice-out and call the functions below, which use the same order. */
#define FDSP_MIX_SUM 1
#define FDSP_MIX_PAN 2
/* EFFECT BANKS.  The lane-per-frame families -- reverb_stereo, reverb4_stereo, fdsp_fdn_create, reverb3_stereo, fdsp_fdn_network_create,
 * fdsp_feedback_delay_create -- mix as well (resynthesizer and convolver banks answer FDSP_ENOTSUP).  One wave of their kernels owns one instance, so the reduction is a
 * launch of its own: the instances render PLANAR into a scratch the bank owns, chunk by chunk (whole 64-frame blocks, "fx_mix_chunk_frames"),
 * a kernel adds every group of 64 instances into the partial-mix buffer in the order above, and the tree runs once at the end; no output
 * transpose and no full-length output exist.  The bus (fdsp_bank_set_bus) is part of the render, so the mix is the mix of the bussed output.
 * fdsp_bank_process_mix takes d_in voice-minor [inputs][frames][instances]; fdsp_bank_process_mix_planar takes it planar
 * [instances][inputs][frame_stride] -- these kernels' native layout; a launch that fits one chunk reads it in place -- and gives the same
 * bits; voice banks answer FDSP_ENOTSUP to it.  FDSP_MIX_PAN pans one-output banks (fdsp_bank_set_pan).
 * The scratch follows the partial-mix buffer's rule: fdsp_bank_mix_reserve(bank, frames) sizes both for launches of up to `frames`; an
 * uncaptured launch that needs more grows them; a captured one is refused (FDSP_EINVAL, reserve first).  The scratch is never shrunk, lives
 * until the bank is destroyed, is apart from the staging copy of fdsp_bank_process, and a clone starts without one. */
int fdsp_bank_process_mix(fdsp_bank* bank, size_t frames, const float* d_in, float* d_mix, int mix, int mode, void* stream);
int fdsp_bank_process_mix_planar(fdsp_bank* bank, size_t frames, const float* d_in, size_t frame_stride, float* d_mix, int mix, int mode, void* stream);
int fdsp_bank_set_pan(fdsp_bank* bank, const float* h_pan, size_t first, size_t count);
int fdsp_bank_mix_reserve(fdsp_bank* bank, size_t frames);

/* The same mix-down of a voice-out render that already sits in HBM.
 * d_voices: [frames][voices] mono voice outputs; d_pan: [voices] pan position in -1..1 or NULL (centre);
 * d_mix: [2][frames].  Equal-power pan weights follow Panner (src/pan.rs:13-17). */
int fdsp_mix_stereo(const float* d_voices, const float* d_pan, float* d_mix, size_t frames, size_t voices,
                    void* stream);

/* Sum over voices of a voice-minor buffer d_in [channels][frames][voices] -> d_out [channels][frames] (per-GPU partial
 * of the mix-down for graphs that already end in a Panner). */
int fdsp_sum_voices(const float* d_in, float* d_out, size_t channels, size_t frames, size_t voices, void* stream);

/* Sum over the instances of a PLANAR render d_in [instances][rows] (rows = channels x frame_stride: reverb_stereo banks, planar
 * voice banks) -> d_out [rows]: the aligned binary tree of the summation order above, taken over the instances. */
int fdsp_sum_instances(const float* d_in, float* d_out, size_t rows, size_t instances, void* stream);

/* ---- the exchange step across GPUs: all-reduce(sum) of the per-GPU partial mixes over RCCL / xGMI ----
 * The only collective of the path: `count` = 2 * frames floats per GPU, latency-bound, issued once per launch.  It runs
 * on the communicator's own side stream, ordered behind the work already queued on `after_stream` (the mix kernel), so
 * the render stream can start the next launch immediately; consumers order themselves behind it with fdsp_comm_wait.
 *   one process, n GPUs:        fdsp_comm_create_local(n, devices, &comm) (devices NULL = 0..n-1); slot k <-> devices[k];
 *                               one thread per GPU calls fdsp_mix_allreduce(comm, k, ..), or one thread calls
 *                               fdsp_mix_allreduce_all(comm, mixes, count, streams) (the calls are grouped)
 *   one process per GPU:        rank 0: fdsp_comm_unique_id(id); ship the 128 bytes to the other ranks (MPI, a file,
 *                               torch.distributed ...); every rank: fdsp_comm_create_rank(id, nranks, rank, device, &comm);
 *                               slot is always 0.
 * The sum is in place in d_mix.  Summation order across GPUs is RCCL's (ring / tree): compare mixes with a tolerance,
 * voices bit for bit (SURVEY 8e parity caveat). */
#define FDSP_COMM_ID_BYTES 128
typedef struct fdsp_comm fdsp_comm;
int fdsp_comm_create_local(int n, const int* devices, fdsp_comm** out);
int fdsp_comm_unique_id(void* id128);
int fdsp_comm_create_rank(const void* id128, int nranks, int rank, int device, fdsp_comm** out);
void fdsp_comm_destroy(fdsp_comm* comm);
int fdsp_comm_ranks(const fdsp_comm* comm);        /* ranks of the whole communicator */
int fdsp_comm_local_slots(const fdsp_comm* comm);  /* ranks owned by this process */
int fdsp_comm_device(const fdsp_comm* comm, int slot);
int fdsp_mix_allreduce(fdsp_comm* comm, int slot, float* d_mix, size_t count, void* after_stream);
int fdsp_mix_allreduce_all(fdsp_comm* comm, float* const* d_mix, size_t count, void* const* after_streams);
int fdsp_comm_wait(fdsp_comm* comm, int slot, void* stream); /* stream == NULL: block the host */

/* ---- shared wavetables (Arc<Wavetable> singletons of the reference: saw_table/square_table/triangle_table,
 * src/wavetable.rs:493-560).  `set`: 0 = saw, 1 = square, 2 = triangle, 4 = organ, 5 = soft saw,
 * 6 = hammond (organ_table/soft_saw_table/hammond_table :546-623), 3 and 7 = user.  Tables are a list of
 * (pitch, power-of-two-length wave) pairs in ascending pitch, data concatenated.  fdsp_wavetable_build() generates the
 * built-in shape with the engine's own make_wave (wavetable.rs:44-123); fdsp_wavetable_upload() installs caller data
 * (e.g. tables produced by FunDSP itself).  Must be called before rendering a kind that uses the set. */
int fdsp_wavetable_build(int set);
int fdsp_wavetable_upload(int set, int n_tables, const float* h_pitches, const int* h_lengths, const float* h_data);
/* Shared sample buffers = the reference's Arc<Wave> handed to playwave() / playwave_at() (src/wave.rs:739-797,
 * prelude32.rs:2225-2248): `slot` 0..7, data [channels][length] f32.  The WavePlayer<slot> node of a graph reads it. */
int fdsp_wave_upload(int slot, int channels, size_t length, const float* h_data);
int fdsp_wavetable_get(int set, int* n_tables, float* h_pitches, int* h_lengths, float* h_data, size_t capacity);
/* The tables fdsp_wavetable_build(set) would install, computed on the host and returned without touching a device
 * (Wavetable::new + make_wave, wavetable.rs:44-123: f64 partial weights, f32 polar insert, f32 radix-2 inverse FFT,
 * f32 peak normalisation).  Bit-identical to the oracle's restatement (tests/test_wavetable_build.py); versus a
 * double-precision FFT of the same spectrum they differ by < 1e-6.  Pass NULL data to query n_tables / lengths. */
int fdsp_wavetable_compute(int set, int* n_tables, float* h_pitches, int* h_lengths, float* h_data, size_t capacity);

/* ---- host-side helpers that restate reference coefficient constructors with the engine's own math --------- */
int fdsp_svf_coefs(int mode, float sample_rate, float cutoff, float q, float gain, float* out6);     /* svf.rs:28-221 */
int fdsp_biquad_coefs(int kind, float sample_rate, float f, float q, float gain, float* out5);       /* biquad.rs:27-116 */
double fdsp_rnd1(uint64_t x);  /* math.rs:569-576 */
/* the engine's restatement of libm::sinf / cosf (lib.rs:470-492) for host-side parameter derivation, e.g. the matrix of
 * rotate(angle, gain) (prelude32.rs:2432) or pan weights */
float fdsp_libm_sinf(float x);
float fdsp_libm_cosf(float x);
uint64_t fdsp_hash1(uint64_t x); /* math.rs:592-599 */

#ifdef __cplusplus
}
#endif
#endif
