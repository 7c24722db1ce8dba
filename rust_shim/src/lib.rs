//! `HipBank`: V voices of one FunDSP graph rendered by the MI355X engine, behind the reference's own `AudioNode` trait.
//!
//! The trait surface, the combinators, `Net` and `Wave::render` stay in Rust (BASELINE.json north_star); what moves is
//! `AudioNode::process` of the voices.  A bank of `V` voices with `I` inputs and `O` outputs per voice is an `AudioNode`
//! with `V * I` inputs and `V * O` outputs: `BufferRef` / `BufferMut` are planar `[channel][64] f32`
//! (src/buffer.rs:8-12), which is exactly `FDSP_LAYOUT_PLANAR` with `frame_stride = 64` when the channels are ordered
//! voice-major -- the slices are handed over without repacking.
//!
//! ```ignore
//! use fundsp::prelude32::*;
//! use fundsp_hip::HipBank;
//! // 512 voices of the README's FM patch; the graph TYPE is compiled for the device from its own type name
//! let voice = sine_hz(110.0) * 110.0 * 2.0 + 110.0 >> sine() >> lowpass_hz(900.0, 1.0);
//! let mut bank: HipBank<U0, U512> = HipBank::from_graph(&voice, 512).unwrap();
//! bank.set_param("0.0.0.0.0.0:value[0]", &freqs).unwrap();          // per-voice field values, by slot
//! let wave = Wave::render(48000.0, 1.0, &mut An(bank));              // unchanged executor: 64-sample process() blocks
//! ```

use core::ffi::{c_char, c_int, c_void};
use core::marker::PhantomData;
use fundsp::prelude32::*;
use std::ffi::{CStr, CString};

pub mod ffi {
    //! `extern "C"` mirror of include/fundsp_hip.h (the subset the shim uses; same names, same argument order).
    use super::*;

    #[repr(C)]
    pub struct FdspBank {
        _private: [u8; 0],
    }
    #[repr(C)]
    pub struct FdspComm {
        _private: [u8; 0],
    }
    /// `struct fdsp_fdn_network` (fdsp_fdn_network_create): a filtered / per-instance Hadamard network
    #[repr(C)]
    pub struct FdspFdnNetwork {
        pub lines: c_int,
        pub inputs: c_int,
        pub outputs: c_int,
        pub taps: c_int,
        pub filter: c_int,
        pub svf_mode: c_int,
        pub place: c_int,
        pub per_instance: c_int,
        pub delays: *const f64,
        pub weights: *const f32,
        pub cutoff: *const f32,
        pub q: *const f32,
        pub gain: *const f32,
        pub line_gain: *const f32,
    }
    /// `struct fdsp_feedback_delay` (fdsp_feedback_delay_create): the identity feedback around one or two delay lines
    #[repr(C)]
    pub struct FdspFeedbackDelay {
        pub channels: c_int,
        pub taps: c_int,
        pub filter: c_int,
        pub svf_mode: c_int,
        pub place: c_int,
        pub reverse: c_int,
        pub per_instance: c_int,
        pub delays: *const f64,
        pub weights: *const f32,
        pub cutoff: *const f32,
        pub q: *const f32,
        pub gain: *const f32,
        pub line_gain: *const f32,
        pub outer_gain: *const f32,
    }
    /// `struct fdsp_resynth_spec` (fdsp_resynth_create): a resynthesizer with a stock processing closure
    #[repr(C)]
    pub struct FdspResynthSpec {
        pub window_length: c_int,
        pub inputs: c_int,
        pub outputs: c_int,
        pub processor: c_int,
        pub source: [c_int; 8],
        pub per_instance: c_int,
        pub flush_denormals: c_int,
        pub lo_hz: *const f32,
        pub hi_hz: *const f32,
        pub gain: *const f32,
    }
    /// `struct fdsp_resynth_fn_spec` (fdsp_resynth_fn_create): a resynthesizer with the caller's closure as a C++ functor in source form
    #[repr(C)]
    pub struct FdspResynthFnSpec {
        pub window_length: c_int,
        pub inputs: c_int,
        pub outputs: c_int,
        pub params: c_int,
        pub state: c_int,
        pub flush_denormals: c_int,
        pub functor: *const c_char,
        pub source: *const c_char,
        pub param_values: *const f32,
    }
    /// `struct fdsp_convolve_spec` (fdsp_convolve_create): convolvers by partitioned FFT convolution, one response row per channel
    #[repr(C)]
    pub struct FdspConvolveSpec {
        pub channels: c_int,
        pub max_len: usize,
        pub len: usize,
        pub per_instance: c_int,
        pub flush_denormals: c_int,
        pub response: *const f32,
    }
    pub const FDSP_RESYNTH_PASS: c_int = 0;
    pub const FDSP_RESYNTH_BAND: c_int = 1;
    pub const FDSP_RESYNTH_GAIN: c_int = 2;
    pub const FDSP_FDN_FILTER_NONE: c_int = 0;
    pub const FDSP_FDN_FILTER_LOWPOLE: c_int = 1;
    pub const FDSP_FDN_FILTER_SVF: c_int = 2;
    pub const FDSP_FDN_IN_LINE: c_int = 0;
    pub const FDSP_FDN_IN_LOOP: c_int = 1;
    pub const FDSP_OK: c_int = 0;
    pub const FDSP_LAYOUT_VOICE_MINOR: c_int = 0;
    pub const FDSP_LAYOUT_PLANAR: c_int = 1;
    pub const FDSP_MODE_PROCESS: c_int = 0;
    pub const FDSP_MODE_TICK: c_int = 1;
    pub const FDSP_MATH_EXACT: c_int = 0;
    pub const FDSP_MATH_FAST: c_int = 1;
    pub const FDSP_SVF_SERIAL: c_int = 0;
    pub const FDSP_SVF_PARALLEL: c_int = 1;
    pub const FDSP_MIX_SUM: c_int = 1;
    pub const FDSP_MIX_PAN: c_int = 2;

    #[link(name = "fundsp_hip")]
    unsafe extern "C" {
        pub fn fdsp_last_error() -> *const c_char;
        pub fn fdsp_device_count() -> c_int;
        pub fn fdsp_kind_by_name(name: *const c_char) -> c_int;
        pub fn fdsp_graph_compile_rust(name: *const c_char, rust_type_name: *const c_char, hints: *const c_char, source: *const c_char) -> c_int;
        pub fn fdsp_bank_create_on(device: c_int, kind: *const c_char, voices: usize, ring_frames: usize, out: *mut *mut FdspBank) -> c_int;
        pub fn fdsp_reverb_stereo_create_on(device: c_int, instances: usize, room_size: f64, time: f64, damping: f64, out: *mut *mut FdspBank) -> c_int;
        pub fn fdsp_reverb4_stereo_create_on(device: c_int, instances: usize, room_size: f64, time: f64, out: *mut *mut FdspBank) -> c_int;
        pub fn fdsp_reverb4_stereo_delays_create_on(device: c_int, instances: usize, delays: *const f32, per_instance: c_int, time: f64, out: *mut *mut FdspBank) -> c_int;
        pub fn fdsp_reverb4_set_delays(bank: *mut FdspBank, delays: *const f32, first: usize, count: usize) -> c_int;
        pub fn fdsp_bank_fitness_reserve(bank: *mut FdspBank) -> c_int;
        pub fn fdsp_bank_reverb_fitness(bank: *mut FdspBank, d_fitness: *mut f32, d_terms: *mut f32, stream: *mut c_void) -> c_int;
        pub fn fdsp_reverb3_stereo_create_on(device: c_int, instances: usize, time: f64, diffusion: f64, lowpole_cutoff_hz: f32, out: *mut *mut FdspBank) -> c_int;
        pub fn fdsp_reverb3_stereo_svf_create_on(device: c_int, instances: usize, time: f64, diffusion: f64, svf_mode: c_int, cutoff_hz: f32, q: f32, gain: f32, out: *mut *mut FdspBank) -> c_int;
        pub fn fdsp_fdn_create_on(device: c_int, instances: usize, lines: c_int, delays: *const f64, taps: c_int, weights: *const f32, inputs: c_int, outputs: c_int, out: *mut *mut FdspBank) -> c_int;
        pub fn fdsp_fdn_network_create_on(device: c_int, instances: usize, net: *const FdspFdnNetwork, sample_rate: f64, out: *mut *mut FdspBank) -> c_int;
        pub fn fdsp_feedback_delay_create_on(device: c_int, instances: usize, net: *const FdspFeedbackDelay, sample_rate: f64, out: *mut *mut FdspBank) -> c_int;
        pub fn fdsp_resynth_create_on(device: c_int, instances: usize, spec: *const FdspResynthSpec, out: *mut *mut FdspBank) -> c_int;
        pub fn fdsp_resynth_fn_create_on(device: c_int, instances: usize, spec: *const FdspResynthFnSpec, out: *mut *mut FdspBank) -> c_int;
        pub fn fdsp_resynth_set_params(bank: *mut FdspBank, values: *const f32, first: usize, count: usize) -> c_int;
        pub fn fdsp_resynth_set_band(bank: *mut FdspBank, lo_hi: *const f32, first: usize, count: usize) -> c_int;
        pub fn fdsp_resynth_set_gain(bank: *mut FdspBank, gain: *const f32, first: usize, count: usize) -> c_int;
        pub fn fdsp_convolve_create_on(device: c_int, instances: usize, spec: *const FdspConvolveSpec, out: *mut *mut FdspBank) -> c_int;
        pub fn fdsp_convolve_routed_create_on(device: c_int, instances: usize, spec: *const FdspConvolveSpec, inputs: c_int, source: *const c_int, out: *mut *mut FdspBank) -> c_int;
        pub fn fdsp_convolve_matrix_create_on(device: c_int, instances: usize, spec: *const FdspConvolveSpec, inputs: c_int, outputs: c_int, term_input: *const c_int, term_output: *const c_int, out: *mut *mut FdspBank) -> c_int;
        pub fn fdsp_convolve_set_response(bank: *mut FdspBank, response: *const f32, len: usize, first: usize, count: usize) -> c_int;
        pub fn fdsp_bank_destroy(bank: *mut FdspBank);
        pub fn fdsp_bank_clone(bank: *const FdspBank, out: *mut *mut FdspBank) -> c_int; // Clone: slots, rings, sample rate, options, events
        pub fn fdsp_bank_inputs(bank: *const FdspBank) -> c_int;
        pub fn fdsp_bank_outputs(bank: *const FdspBank) -> c_int;
        pub fn fdsp_bank_voices(bank: *const FdspBank) -> usize;
        pub fn fdsp_bank_device(bank: *const FdspBank) -> c_int;
        pub fn fdsp_bank_set_sample_rate(bank: *mut FdspBank, sample_rate: f64) -> c_int; // AudioNode::set_sample_rate
        pub fn fdsp_bank_reset(bank: *mut FdspBank) -> c_int; // AudioNode::reset
        pub fn fdsp_bank_set_seed(bank: *mut FdspBank, seeds: *const u64, first: usize, count: usize) -> c_int; // set_seed / ping
        pub fn fdsp_bank_set_param(bank: *mut FdspBank, name: *const c_char, values: *const f32, first: usize, count: usize) -> c_int;
        pub fn fdsp_bank_set_param_all(bank: *mut FdspBank, name: *const c_char, value: f32) -> c_int;
        pub fn fdsp_bank_set_option(bank: *mut FdspBank, name: *const c_char, value: c_int) -> c_int;
        pub fn fdsp_bank_set_bus(bank: *mut FdspBank, mode: c_int, wet: f32, dry: f32) -> c_int;
        pub fn fdsp_jit_compiler() -> *const c_char;
        pub fn fdsp_bank_slot_count(bank: *const FdspBank) -> c_int;
        pub fn fdsp_bank_get_state(bank: *mut FdspBank, slots: *mut f32) -> c_int; // Clone
        pub fn fdsp_bank_set_state(bank: *mut FdspBank, slots: *const f32) -> c_int;
        pub fn fdsp_bank_process_host(bank: *mut FdspBank, frames: usize, input: *const f32, output: *mut f32, layout: c_int,
                                      frame_stride: usize, mode: c_int) -> c_int; // AudioNode::process on host buffers
        pub fn fdsp_bank_process(bank: *mut FdspBank, frames: usize, d_in: *const f32, d_out: *mut f32, layout: c_int,
                                 frame_stride: usize, mode: c_int, stream: *mut c_void) -> c_int; // device-resident I/O
        pub fn fdsp_bank_process_mix(bank: *mut FdspBank, frames: usize, d_in: *const f32, d_mix: *mut f32, mix: c_int, mode: c_int,
                                     stream: *mut c_void) -> c_int; // render + reduce over the voices in one launch
        pub fn fdsp_bank_process_mix_planar(bank: *mut FdspBank, frames: usize, d_in: *const f32, frame_stride: usize, d_mix: *mut f32, mix: c_int,
                                            mode: c_int, stream: *mut c_void) -> c_int; // effect banks: the same from a planar input
        pub fn fdsp_bank_process_events_mix(bank: *mut FdspBank, frames: usize, d_in: *const f32, d_mix: *mut f32, mode: c_int, stream: *mut c_void) -> c_int; // Sequencer output
        pub fn fdsp_bank_set_score(bank: *mut FdspBank, notes: usize, voice: *const c_int, events: *const f64, fade: *const c_int, nparams: c_int,
                                   names: *const *const c_char, params: *const f32) -> c_int; // many notes per voice
        pub fn fdsp_bank_set_pan(bank: *mut FdspBank, pan: *const f32, first: usize, count: usize) -> c_int;
        pub fn fdsp_bank_mix_reserve(bank: *mut FdspBank, frames: usize) -> c_int; // AudioNode::allocate for the mix path
        pub fn fdsp_bank_synchronize(bank: *mut FdspBank) -> c_int;
        pub fn fdsp_sum_voices(d_in: *const f32, d_out: *mut f32, channels: usize, frames: usize, voices: usize, stream: *mut c_void) -> c_int;
        pub fn fdsp_sum_instances(d_in: *const f32, d_out: *mut f32, rows: usize, instances: usize, stream: *mut c_void) -> c_int;
        pub fn fdsp_mix_stereo(d_voices: *const f32, d_pan: *const f32, d_mix: *mut f32, frames: usize, voices: usize, stream: *mut c_void) -> c_int;
        pub fn fdsp_comm_create_local(n: c_int, devices: *const c_int, out: *mut *mut FdspComm) -> c_int;
        pub fn fdsp_comm_unique_id(id128: *mut c_void) -> c_int;
        pub fn fdsp_comm_create_rank(id128: *const c_void, nranks: c_int, rank: c_int, device: c_int, out: *mut *mut FdspComm) -> c_int;
        pub fn fdsp_comm_destroy(comm: *mut FdspComm);
        pub fn fdsp_mix_allreduce(comm: *mut FdspComm, slot: c_int, d_mix: *mut f32, count: usize, after_stream: *mut c_void) -> c_int;
        pub fn fdsp_comm_wait(comm: *mut FdspComm, slot: c_int, stream: *mut c_void) -> c_int;
    }
}
use ffi::*;

/// The network of `HipBank::fdn_network` (see there): filter = FDSP_FDN_FILTER_*, svf_mode = FDSP_SVF_* order (0 lowpass .. 8 highshelf),
/// place = FDSP_FDN_IN_LINE | FDSP_FDN_IN_LOOP; `taps` = 0 means no Fir node, `line_gain` = None no `* g` node.
pub struct FdnNetwork<'a> {
    pub inputs: usize,
    pub outputs: usize,
    pub taps: usize,
    pub filter: c_int,
    pub svf_mode: c_int,
    pub place: c_int,
    pub per_instance: bool,
    pub delays: &'a [f64],
    pub weights: &'a [f32],
    pub cutoff: Option<&'a [f32]>,
    pub q: Option<&'a [f32]>,
    pub gain: Option<&'a [f32]>,
    pub line_gain: Option<&'a [f32]>,
}

/// The network of `HipBank::feedback_delay` (see there): filter = FDSP_FDN_FILTER_*, svf_mode = FDSP_SVF_* order, place = FDSP_FDN_IN_LINE
/// (`feedback`) | FDSP_FDN_IN_LOOP (`feedback2`); `taps` = 0 means no Fir node, `line_gain` / `outer_gain` = None no such `* g` node.
pub struct FeedbackDelay<'a> {
    pub channels: usize,
    pub taps: usize,
    pub filter: c_int,
    pub svf_mode: c_int,
    pub place: c_int,
    pub reverse: bool,
    pub per_instance: bool,
    pub delays: &'a [f64],
    pub weights: &'a [f32],
    pub cutoff: Option<&'a [f32]>,
    pub q: Option<&'a [f32]>,
    pub gain: Option<&'a [f32]>,
    pub line_gain: Option<&'a [f32]>,
    pub outer_gain: Option<&'a [f32]>,
}

/// The engine's last error message for this thread.
pub fn last_error() -> String {
    unsafe { CStr::from_ptr(fdsp_last_error()).to_string_lossy().into_owned() }
}

fn check(rc: c_int) -> Result<(), String> {
    if rc == FDSP_OK { Ok(()) } else { Err(last_error()) }
}

/// A bank of voices on one GPU.  `NI` = voices x inputs per voice, `NO` = voices x outputs per voice (typenum sizes, as
/// every `AudioNode` declares them).
///
/// The `AudioNode` face has a practical ceiling: `tick()` builds `Frame<f32, NO>` on the stack (a `GenericArray`: 4 B per
/// channel -- 256 KB at `U65536`) and every combinator above the bank instantiates typenum arithmetic over `NI` / `NO`.  The
/// reference uses `Size` at channel counts of tens (`U32` in its FDN reverbs, src/prelude.rs:1732-1762); use the trait face at
/// bank sizes of that order (a few hundred voices at most) and [`HipBank::render_device`] / [`HipBank::render_mix`] for the
/// BASELINE-sized banks, where `NI` / `NO` are only the arity check of `new` (pass `U0` and skip it with `new_unchecked_arity`).
pub struct HipBank<NI: Size<f32>, NO: Size<f32>> {
    bank: *mut FdspBank,
    kind: CString,
    voices: usize,
    ring_frames: usize,
    device: c_int,
    /// `tick` / `process` are infallible in FunDSP.  A failed launch (lost device, wrong arity) zeroes the output and is
    /// recorded here -- in release builds too -- for the host to poll with `take_error()`.
    last_error: Option<String>,
    /// terms of a summing convolver bank ([`Self::convolve_matrix`]: its response rows are per term, not per output), else 0
    convolve_terms: usize,
    _marker: PhantomData<(NI, NO)>,
}

// The handle may move between threads and is used by one thread at a time (`process(&mut self)`); `&self` methods do
// not touch the device.
unsafe impl<NI: Size<f32>, NO: Size<f32>> Send for HipBank<NI, NO> {}
unsafe impl<NI: Size<f32>, NO: Size<f32>> Sync for HipBank<NI, NO> {}

impl<NI: Size<f32>, NO: Size<f32>> HipBank<NI, NO> {
    /// `voices` instances of an ahead-of-time kind ("fm_svf", "fixed_svf", "biquad_bank" ...) on `device` (-1 = current).
    pub fn new(kind: &str, voices: usize, ring_frames: usize, device: i32) -> Result<Self, String> {
        let kind = CString::new(kind).map_err(|e| e.to_string())?;
        let mut bank: *mut FdspBank = core::ptr::null_mut();
        check(unsafe { fdsp_bank_create_on(device as c_int, kind.as_ptr(), voices, ring_frames, &mut bank) })?;
        let (i, o) = unsafe { (fdsp_bank_inputs(bank) as usize, fdsp_bank_outputs(bank) as usize) };
        if i * voices != NI::USIZE || o * voices != NO::USIZE {
            unsafe { fdsp_bank_destroy(bank) };
            return Err(format!("arity mismatch: the bank has {}x{} inputs and {}x{} outputs", voices, i, voices, o));
        }
        let device = unsafe { fdsp_bank_device(bank) };
        Ok(Self { bank, kind, voices, ring_frames, device, last_error: None, convolve_terms: 0, _marker: PhantomData })
    }

    /// The same without the typenum arity check: for banks far beyond the channel counts `Size` is meant for (65 536 voices),
    /// which are driven through `render_device` / `render_mix` only.  `tick` / `process` of such a bank report an arity error.
    pub fn new_unchecked_arity(kind: &str, voices: usize, ring_frames: usize, device: i32) -> Result<Self, String> {
        let kind = CString::new(kind).map_err(|e| e.to_string())?;
        let mut bank: *mut FdspBank = core::ptr::null_mut();
        check(unsafe { fdsp_bank_create_on(device as c_int, kind.as_ptr(), voices, ring_frames, &mut bank) })?;
        let device = unsafe { fdsp_bank_device(bank) };
        Ok(Self { bank, kind, voices, ring_frames, device, last_error: None, convolve_terms: 0, _marker: PhantomData })
    }

    /// `instances` x `reverb_stereo(room_size, time, damping)` (src/prelude.rs:1732-1762) through the dedicated lane-per-frame FDN kernel
    /// (one wave per instance, the 32 delay lines in registers) instead of the generic lane-per-voice `Feedback` kernel `from_graph` builds
    /// for the same type: bit-identical output, an order of magnitude faster.  Each instance has two inputs and two outputs.
    pub fn reverb_stereo(instances: usize, room_size: f64, time: f64, damping: f64, device: i32) -> Result<Self, String> {
        let mut bank: *mut FdspBank = core::ptr::null_mut();
        check(unsafe { fdsp_reverb_stereo_create_on(device as c_int, instances, room_size, time, damping, &mut bank) })?;
        Self::adopt(bank, "reverb_stereo", instances)
    }

    /// `instances` x `reverb4_stereo(room_size, time)` (src/prelude.rs:1873-1941: two 16-line Hadamard networks in series), same kernel family.
    pub fn reverb4_stereo(instances: usize, room_size: f64, time: f64, device: i32) -> Result<Self, String> {
        let mut bank: *mut FdspBank = core::ptr::null_mut();
        check(unsafe { fdsp_reverb4_stereo_create_on(device as c_int, instances, room_size, time, &mut bank) })?;
        Self::adopt(bank, "reverb4_stereo", instances)
    }

    /// `instances` x `reverb4_stereo_delays(delays, time)` (src/prelude.rs:1917-1941): `delays` holds 32 times for the whole bank or
    /// `instances` x 32 for a table per instance -- the candidates of examples/optimize.rs (src/reverb.rs:17-28) in one bank.
    pub fn reverb4_stereo_delays(instances: usize, delays: &[f32], time: f64, device: i32) -> Result<Self, String> {
        if delays.len() != 32 && delays.len() != instances * 32 {
            return Err("HipBank::reverb4_stereo_delays: delays needs 32 or instances x 32 times".into());
        }
        let per_instance = (delays.len() != 32) as c_int;
        let mut bank: *mut FdspBank = core::ptr::null_mut();
        check(unsafe { fdsp_reverb4_stereo_delays_create_on(device as c_int, instances, delays.as_ptr(), per_instance, time, &mut bank) })?;
        Self::adopt(bank, "reverb4_stereo", instances)
    }

    /// Replace the delay rows `first` .. of a `reverb4_stereo_delays` bank (`delays` holds count x 32 times) and reset their instances.
    pub fn set_delays(&mut self, delays: &[f32], first: usize) -> Result<(), String> {
        if delays.is_empty() || delays.len() % 32 != 0 {
            return Err("HipBank::set_delays: delays needs count x 32 times".into());
        }
        check(unsafe { fdsp_reverb4_set_delays(self.bank, delays.as_ptr(), first, delays.len() / 32) })
    }

    /// `AudioNode::allocate` for `reverb_fitness`: the call then allocates nothing.
    pub fn fitness_reserve(&mut self) -> Result<(), String> { check(unsafe { fdsp_bank_fitness_reserve(self.bank) }) }

    /// `reverb_fitness` (src/reverb.rs:31-139) of every instance of a stereo effect bank, on the device: `d_fitness` = [instances] device
    /// floats, `d_terms` NULL or [instances][4] (echo_0, pen_0, echo_1, pen_1).  The bank is reset before and after.
    pub fn reverb_fitness(&mut self, d_fitness: *mut f32, d_terms: *mut f32, stream: *mut c_void) -> Result<(), String> {
        check(unsafe { fdsp_bank_reverb_fitness(self.bank, d_fitness, d_terms, stream) })
    }

    /// `instances` x `reverb3_stereo(time, diffusion, lowpole_hz(cutoff))` (src/prelude.rs:1858-1871; `Reverb<F>`, src/reverb.rs:152-279) through its
    /// lane-per-frame kernel: bit-identical to the `Reverb3` node `from_graph` builds for the type, two orders of magnitude faster.
    pub fn reverb3_stereo(instances: usize, time: f64, diffusion: f64, lowpole_cutoff_hz: f32, device: i32) -> Result<Self, String> {
        let mut bank: *mut FdspBank = core::ptr::null_mut();
        check(unsafe { fdsp_reverb3_stereo_create_on(device as c_int, instances, time, diffusion, lowpole_cutoff_hz, &mut bank) })?;
        Self::adopt(bank, "reverb3_stereo", instances)
    }

    /// ... with a `FixedSvf` as the loop filter: `svf_mode` 0..8 = lowpass, highpass, bandpass, notch, peak, allpass, bell, lowshelf, highshelf
    /// (`reverb3_stereo(time, diffusion, highshelf_hz(5000.0, 1.0, db_amp(-1.0)))` of examples/keys.rs:134 is mode 8).
    pub fn reverb3_stereo_svf(instances: usize, time: f64, diffusion: f64, svf_mode: i32, cutoff_hz: f32, q: f32, gain: f32, device: i32) -> Result<Self, String> {
        let mut bank: *mut FdspBank = core::ptr::null_mut();
        check(unsafe { fdsp_reverb3_stereo_svf_create_on(device as c_int, instances, time, diffusion, svf_mode as c_int, cutoff_hz, q, gain, &mut bank) })?;
        Self::adopt(bank, "reverb3_stereo", instances)
    }

    /// `instances` x the Hadamard feedback delay network of the prelude's own example (src/prelude.rs:1323-1345):
    /// `split::<N>() >> fdn::<N, _>(stacki::<N, _, _>(|i| delay(delays[i]) >> fir(weights))) >> join::<N>()` with `inputs = outputs = 1`,
    /// `multisplit::<U2, _>` / `multijoin::<U2, _>` around it with 2.  `delays.len()` = N in 2, 4, 8, 16, 32; one to three FIR weights; every
    /// delay longer than 128 samples at the bank's sample rate.  Same kernel family as the reverbs: bit-identical to the `Feedback` graph
    /// `from_graph` would build for the type, two orders of magnitude faster.
    pub fn fdn(instances: usize, delays: &[f64], weights: &[f32], inputs: usize, outputs: usize, device: i32) -> Result<Self, String> {
        let mut bank: *mut FdspBank = core::ptr::null_mut();
        check(unsafe {
            fdsp_fdn_create_on(device as c_int, instances, delays.len() as c_int, delays.as_ptr(), weights.len() as c_int, weights.as_ptr(), inputs as c_int, outputs as c_int, &mut bank)
        })?;
        Self::adopt(bank, "fdn", instances)
    }

    /// `instances` x a Hadamard network with a filter in its lines (`place` = FDSP_FDN_IN_LINE:
    /// `fdn(stacki(|i| delay(t_i) [>> fir(w_i)] [>> F_i] [* g_i]))`) or in its loop (FDSP_FDN_IN_LOOP:
    /// `fdn2(stacki(|i| delay(t_i) [>> fir(w_i)]), stacki(|i| F_i [* g_i]))`), split / multisplit in front and join / multijoin behind
    /// (include/fundsp_hip.h `fdsp_fdn_network`).  Every slice holds one value per line, or with `per_instance` one per instance and line
    /// (`weights`: `taps` per line); the bank is created at `sample_rate`, where every delay must be at least 128 samples.
    pub fn fdn_network(instances: usize, net: &FdnNetwork, sample_rate: f64, device: i32) -> Result<Self, String> {
        let sets = if net.per_instance { instances } else { 1 };
        let lines = if sets == 0 { 0 } else { net.delays.len() / sets };
        let per_line = |a: Option<&[f32]>, k: usize| a.map_or(true, |a| a.len() == sets * lines * k);
        if lines * sets != net.delays.len() || !per_line(Some(net.weights), net.taps) || !per_line(net.cutoff, 1) || !per_line(net.q, 1)
            || !per_line(net.gain, 1) || !per_line(net.line_gain, 1)
        {
            return Err("HipBank::fdn_network: every slice needs one value per line (per instance and line with per_instance)".into());
        }
        let ptr = |a: Option<&[f32]>| a.map_or(core::ptr::null(), |a| a.as_ptr());
        let c = FdspFdnNetwork {
            lines: lines as c_int,
            inputs: net.inputs as c_int,
            outputs: net.outputs as c_int,
            taps: net.taps as c_int,
            filter: net.filter,
            svf_mode: net.svf_mode,
            place: net.place,
            per_instance: net.per_instance as c_int,
            delays: net.delays.as_ptr(),
            weights: if net.taps > 0 { net.weights.as_ptr() } else { core::ptr::null() },
            cutoff: ptr(net.cutoff),
            q: ptr(net.q),
            gain: ptr(net.gain),
            line_gain: ptr(net.line_gain),
        };
        let mut bank: *mut FdspBank = core::ptr::null_mut();
        check(unsafe { fdsp_fdn_network_create_on(device as c_int, instances, &c, sample_rate, &mut bank) })?;
        Self::adopt(bank, "fdn_network", instances)
    }

    /// `instances` x the identity feedback around one or two delay lines (include/fundsp_hip.h `fdsp_feedback_delay`): the echo
    /// `feedback(delay(t) * g)`, the ping-pong `feedback((delay(t) | delay(t)) >> reverse() * g)`, combs with `lowpole_hz` or a `FixedSvf` in
    /// the line (`place` = FDSP_FDN_IN_LINE) or in `feedback2`'s loop (FDSP_FDN_IN_LOOP).  Every slice holds one value per channel, or with
    /// `per_instance` one per instance and channel (`weights`: `taps` per channel; `outer_gain`: one per bank or per instance); the bank is
    /// created at `sample_rate`, where every delay must be at least 128 samples.  Source only: no Rust toolchain has built it.
    pub fn feedback_delay(instances: usize, net: &FeedbackDelay, sample_rate: f64, device: i32) -> Result<Self, String> {
        let sets = if net.per_instance { instances } else { 1 };
        let n = net.channels;
        let per_line = |a: Option<&[f32]>, k: usize| a.map_or(true, |a| a.len() == sets * n * k);
        if net.delays.len() != sets * n || !per_line(Some(net.weights), net.taps) || !per_line(net.cutoff, 1) || !per_line(net.q, 1)
            || !per_line(net.gain, 1) || !per_line(net.line_gain, 1) || net.outer_gain.map_or(false, |a| a.len() != sets)
        {
            return Err("HipBank::feedback_delay: every slice needs one value per channel (per instance and channel with per_instance)".into());
        }
        let ptr = |a: Option<&[f32]>| a.map_or(core::ptr::null(), |a| a.as_ptr());
        let c = FdspFeedbackDelay {
            channels: n as c_int,
            taps: net.taps as c_int,
            filter: net.filter,
            svf_mode: net.svf_mode,
            place: net.place,
            reverse: net.reverse as c_int,
            per_instance: net.per_instance as c_int,
            delays: net.delays.as_ptr(),
            weights: if net.taps > 0 { net.weights.as_ptr() } else { core::ptr::null() },
            cutoff: ptr(net.cutoff),
            q: ptr(net.q),
            gain: ptr(net.gain),
            line_gain: ptr(net.line_gain),
            outer_gain: ptr(net.outer_gain),
        };
        let mut bank: *mut FdspBank = core::ptr::null_mut();
        check(unsafe { fdsp_feedback_delay_create_on(device as c_int, instances, &c, sample_rate, &mut bank) })?;
        Self::adopt(bank, "feedback_delay", instances)
    }

    /// `instances` x `resynth::<I, O, _>(window_length, closure)` (src/resynth.rs) with a stock closure (include/fundsp_hip.h
    /// `fdsp_resynth_spec`): `processor` = FDSP_RESYNTH_PASS (`fft.set(o, i, fft.at(source[o], i))`), FDSP_RESYNTH_BAND (the same where
    /// lo_hz[o] <= fft.frequency(i) <= hi_hz[o]) or FDSP_RESYNTH_GAIN (times gain[o][i], window_length / 2 + 1 bins per output).  `source[o]`:
    /// the input channel of output o, -1 = silent.  Tables hold one row, or with `per_instance` one per instance.  `flush_denormals` when a
    /// Feedback node was constructed in front of the node (the reference then renders it flushed).  Source only: no Rust toolchain has built it.
    pub fn resynth(instances: usize, window_length: usize, source: &[i32], processor: i32, per_instance: bool, lo_hi: Option<(&[f32], &[f32])>,
                   gain: Option<&[f32]>, inputs: usize, flush_denormals: bool, device: i32) -> Result<Self, String> {
        if source.is_empty() || source.len() > 8 {
            return Err("HipBank::resynth: one source entry per output, 1 .. 8 outputs".into());
        }
        let rows = if per_instance { instances } else { 1 };
        let outputs = source.len();
        if lo_hi.map_or(false, |(l, h)| l.len() != rows * outputs || h.len() != rows * outputs)
            || gain.map_or(false, |g| g.len() != rows * outputs * (window_length / 2 + 1))
        {
            return Err("HipBank::resynth: tables need one row (per instance with per_instance) of one entry per output (gain: per bin)".into());
        }
        let mut src = [-1 as c_int; 8];
        for (o, &s) in source.iter().enumerate() {
            src[o] = s as c_int;
        }
        let spec = FdspResynthSpec {
            window_length: window_length as c_int,
            inputs: inputs as c_int,
            outputs: outputs as c_int,
            processor: processor as c_int,
            source: src,
            per_instance: per_instance as c_int,
            flush_denormals: flush_denormals as c_int,
            lo_hz: lo_hi.map_or(core::ptr::null(), |(l, _)| l.as_ptr()),
            hi_hz: lo_hi.map_or(core::ptr::null(), |(_, h)| h.as_ptr()),
            gain: gain.map_or(core::ptr::null(), |g| g.as_ptr()),
        };
        let mut bank: *mut FdspBank = core::ptr::null_mut();
        check(unsafe { fdsp_resynth_create_on(device as c_int, instances, &spec, &mut bank) })?;
        Self::adopt(bank, "resynth", instances)
    }

    /// `instances` x `resynth::<I, O, _>(window_length, |fft| ...)` with the caller's closure (include/fundsp_hip.h `fdsp_resynth_fn_spec`):
    /// `functor` names a C++ type in namespace fd that `source` defines in the per-bin form of fundsp_amd/csrc/fd_resynth_fn.hpp; `params`
    /// f32 values per instance (`param_values`: [instances][params], empty = zeros) and `state` f32 values per (instance, bin) must equal the
    /// functor's PARAMS / STATE.  Compiled at creation.  Source only: no Rust toolchain has built it.
    pub fn resynth_fn(instances: usize, window_length: usize, inputs: usize, outputs: usize, functor: &str, source: &str, params: usize,
                      state: usize, param_values: &[f32], flush_denormals: bool, device: i32) -> Result<Self, String> {
        if !param_values.is_empty() && param_values.len() != instances * params {
            return Err("HipBank::resynth_fn: param_values takes instances x params values (or none: zeros)".into());
        }
        let functor = CString::new(functor).map_err(|e| e.to_string())?;
        let source = CString::new(source).map_err(|e| e.to_string())?;
        let spec = FdspResynthFnSpec {
            window_length: window_length as c_int,
            inputs: inputs as c_int,
            outputs: outputs as c_int,
            params: params as c_int,
            state: state as c_int,
            flush_denormals: flush_denormals as c_int,
            functor: functor.as_ptr(),
            source: source.as_ptr(),
            param_values: if param_values.is_empty() { core::ptr::null() } else { param_values.as_ptr() },
        };
        let mut bank: *mut FdspBank = core::ptr::null_mut();
        check(unsafe { fdsp_resynth_fn_create_on(device as c_int, instances, &spec, &mut bank) })?;
        Self::adopt(bank, "resynth", instances)
    }

    /// Replace the closure parameters of instances `first ..` (fdsp_resynth_set_params): `values` holds [count][params]; they apply from the next launch.
    pub fn set_resynth_params(&mut self, values: &[f32], first: usize, count: usize) -> Result<(), String> {
        check(unsafe { fdsp_resynth_set_params(self.bank, values.as_ptr(), first, count) })
    }

    /// `instances` x `channels` convolvers, `convolve(&wave, channel)` per channel (src/convolve.rs; include/fundsp_hip.h
    /// `fdsp_convolve_spec`): `response` holds [channels][len], or [instances][channels][len] with `per_instance`; `max_len` is the capacity
    /// [`Self::set_response`] can fill later.  No latency; the bits are the project's own statement (fd_convolve.hpp), not the crate's.
    /// Source only: no Rust toolchain has built it.
    pub fn convolve(instances: usize, channels: usize, response: &[f32], len: usize, max_len: usize, per_instance: bool, flush_denormals: bool,
                    device: i32) -> Result<Self, String> {
        let rows = if per_instance { instances } else { 1 };
        if channels < 1 || channels > 8 || len < 1 || response.len() != rows * channels * len {
            return Err("HipBank::convolve: response needs rows x channels x len taps (rows = instances with per_instance), 1 .. 8 channels".into());
        }
        let spec = FdspConvolveSpec {
            channels: channels as c_int,
            max_len,
            len,
            per_instance: per_instance as c_int,
            flush_denormals: flush_denormals as c_int,
            response: response.as_ptr(),
        };
        let mut bank: *mut FdspBank = core::ptr::null_mut();
        check(unsafe { fdsp_convolve_create_on(device as c_int, instances, &spec, &mut bank) })?;
        Self::adopt(bank, "convolve", instances)
    }

    /// One input through several responses, `convolve(&w, 0) ^ convolve(&w, 1)` (fdsp_convolve_routed_create): a bank of `inputs` inputs
    /// and `source.len()` outputs whose output c convolves input `source[c]` with response row c; `response` as for [`Self::convolve`]
    /// with channels = outputs.  Outputs of one input share its input ring and spectrum ring; the bits are those of [`Self::convolve`] fed
    /// copies of the input rows.  Source only: no Rust toolchain has built it.
    pub fn convolve_routed(instances: usize, inputs: usize, source: &[i32], response: &[f32], len: usize, max_len: usize, per_instance: bool,
                           flush_denormals: bool, device: i32) -> Result<Self, String> {
        let rows = if per_instance { instances } else { 1 };
        let channels = source.len();
        if channels < 1 || channels > 8 || len < 1 || response.len() != rows * channels * len {
            return Err("HipBank::convolve_routed: response needs rows x outputs x len taps (rows = instances with per_instance), 1 .. 8 outputs".into());
        }
        let spec = FdspConvolveSpec {
            channels: channels as c_int,
            max_len,
            len,
            per_instance: per_instance as c_int,
            flush_denormals: flush_denormals as c_int,
            response: response.as_ptr(),
        };
        let src: Vec<c_int> = source.iter().map(|&i| i as c_int).collect();
        let mut bank: *mut FdspBank = core::ptr::null_mut();
        check(unsafe { fdsp_convolve_routed_create_on(device as c_int, instances, &spec, inputs as c_int, src.as_ptr(), &mut bank) })?;
        Self::adopt(bank, "convolve", instances)
    }

    /// Several inputs convolved and added into one output, `convolve(&w, 0) + convolve(&w, 1)` (fdsp_convolve_matrix_create): a bank of
    /// `inputs` inputs, `outputs` outputs and `term_input.len()` terms (1 .. 16); term t convolves input `term_input[t]` with response row
    /// t into output `term_output[t]` (non-decreasing).  `response` as for [`Self::convolve`] with channels = terms.  The terms of an output
    /// are summed before its one inverse transform; an output of one term has the bits of [`Self::convolve_routed`].  A true-stereo
    /// response `(ll + rl) ^ (lr + rr)` is term_input = [0, 1, 0, 1], term_output = [0, 0, 1, 1].  Source only: no Rust toolchain has built it.
    pub fn convolve_matrix(instances: usize, inputs: usize, outputs: usize, term_input: &[i32], term_output: &[i32], response: &[f32], len: usize,
                           max_len: usize, per_instance: bool, flush_denormals: bool, device: i32) -> Result<Self, String> {
        let rows = if per_instance { instances } else { 1 };
        let terms = term_input.len();
        if terms < 1 || terms > 16 || term_output.len() != terms || len < 1 || response.len() != rows * terms * len {
            return Err("HipBank::convolve_matrix: one input and one output index per term, 1 .. 16 terms; response needs rows x terms x len taps (rows = instances with per_instance)".into());
        }
        let spec = FdspConvolveSpec {
            channels: terms as c_int,
            max_len,
            len,
            per_instance: per_instance as c_int,
            flush_denormals: flush_denormals as c_int,
            response: response.as_ptr(),
        };
        let tin: Vec<c_int> = term_input.iter().map(|&i| i as c_int).collect();
        let tout: Vec<c_int> = term_output.iter().map(|&i| i as c_int).collect();
        let mut bank: *mut FdspBank = core::ptr::null_mut();
        check(unsafe { fdsp_convolve_matrix_create_on(device as c_int, instances, &spec, inputs as c_int, outputs as c_int, tin.as_ptr(), tout.as_ptr(), &mut bank) })?;
        let mut b = Self::adopt(bank, "convolve", instances)?;
        b.convolve_terms = terms;
        Ok(b)
    }

    /// Convolver::set_response for rows `first` .. : `response` holds [count][channels][len] (channels = the outputs, or the terms of a
    /// summing bank); the history of the whole bank is cleared
    pub fn set_response(&mut self, response: &[f32], len: usize, first: usize, count: usize) -> Result<(), String> {
        let channels = if self.convolve_terms > 0 { self.convolve_terms } else { unsafe { fdsp_bank_outputs(self.bank) as usize } };
        if response.len() != count * channels * len {
            return Err("HipBank::set_response: response needs count x channels x len taps".into());
        }
        check(unsafe { fdsp_convolve_set_response(self.bank, response.as_ptr(), len, first, count) })
    }

    fn adopt(bank: *mut FdspBank, kind: &str, voices: usize) -> Result<Self, String> {
        let device = unsafe { fdsp_bank_device(bank) };
        Ok(Self { bank, kind: CString::new(kind).unwrap(), voices, ring_frames: 0, device, last_error: None, convolve_terms: 0, _marker: PhantomData })
    }

    fn arity_ok(&self) -> bool {
        let (i, o) = unsafe { (fdsp_bank_inputs(self.bank) as usize, fdsp_bank_outputs(self.bank) as usize) };
        i * self.voices == NI::USIZE && o * self.voices == NO::USIZE
    }

    /// `voices` instances of the graph TYPE `X`: `core::any::type_name::<X>()` goes to the engine's front door
    /// (fdsp_graph_compile_rust), which builds the fused device kernel and remembers the parameters the type carries
    /// (filter modes, shape kinds).  Field values of `_voice` are NOT read: set them per voice with [`Self::set_param`].
    pub fn from_graph<X: AudioNode>(_voice: &An<X>, voices: usize) -> Result<Self, String> {
        Self::from_graph_with::<X>(voices, 0, -1, None, None)
    }

    pub fn from_graph_with<X: AudioNode>(voices: usize, ring_frames: usize, device: i32, hints: Option<&str>,
                                         functor_source: Option<&str>) -> Result<Self, String> {
        let type_name = core::any::type_name::<An<X>>();
        // a stable kind name per graph type
        let mut h = AttoHash::new(0x4849_5042);
        for b in type_name.bytes() {
            h = h.hash(b as u64);
        }
        let name = format!("rust_{:016x}", h.state());
        let cname = CString::new(name.clone()).unwrap();
        let ctype = CString::new(type_name).map_err(|e| e.to_string())?;
        let chints = hints.map(|s| CString::new(s).unwrap());
        let csrc = functor_source.map(|s| CString::new(s).unwrap());
        let rc = unsafe {
            fdsp_graph_compile_rust(cname.as_ptr(), ctype.as_ptr(), chints.as_ref().map_or(core::ptr::null(), |c| c.as_ptr()),
                                    csrc.as_ref().map_or(core::ptr::null(), |c| c.as_ptr()))
        };
        if rc < 0 {
            return Err(last_error());
        }
        Self::new(&name, voices, ring_frames, device)
    }

    pub fn voices(&self) -> usize { self.voices }
    pub fn device(&self) -> i32 { self.device }

    /// The error of a failed `tick` / `process` since the last call (those two cannot return one): `None` = all launches
    /// succeeded.  A failed launch has already zeroed its output block.
    pub fn take_error(&mut self) -> Option<String> { self.last_error.take() }

    /// One value per voice for the named slot (`"<path>:<field>"`, listed by `fdsp_kind_slot_name`): what
    /// `Setting::center(..)`, `.q(..)`, `Constant` values etc. are on a single node.
    pub fn set_param(&mut self, slot: &str, values: &[f32]) -> Result<(), String> {
        let c = CString::new(slot).map_err(|e| e.to_string())?;
        check(unsafe { fdsp_bank_set_param(self.bank, c.as_ptr(), values.as_ptr(), 0, values.len()) })
    }

    pub fn set_param_all(&mut self, slot: &str, value: f32) -> Result<(), String> {
        let c = CString::new(slot).map_err(|e| e.to_string())?;
        check(unsafe { fdsp_bank_set_param_all(self.bank, c.as_ptr(), value) })
    }

    /// `AudioNode::set_seed` per voice (`ping(false, AttoHash::new(seed))`).
    pub fn set_seeds(&mut self, seeds: &[u64]) -> Result<(), String> {
        check(unsafe { fdsp_bank_set_seed(self.bank, seeds.as_ptr(), 0, seeds.len()) })
    }

    /// `dry * multipass() & wet * node` around a reverb / network bank (src/audionode.rs:1842-1877 `Bus`, :1190-1228 `FrameMulScalar`), folded
    /// into the bank's render kernel: README.md:436's `multipass() & 0.2 * reverb_stereo(20.0, 2.0, 1.0)` is `set_bus(Some(1.0), 0.2)`;
    /// `None` for the dry side leaves `wet * node` alone.  Factors of 1.0 are the nodes a graph leaves out (x * 1.0 == x).
    pub fn set_bus(&mut self, dry: Option<f32>, wet: f32) -> Result<(), String> {
        check(unsafe { fdsp_bank_set_bus(self.bank, if dry.is_some() { 2 } else { 1 }, wet, dry.unwrap_or(1.0)) })
    }

    /// Which hiprtc compiles run-time compiled graphs in this process (`"linked: <path>"` for a Rust host; see include/fundsp_hip.h).
    pub fn jit_compiler() -> String {
        unsafe { std::ffi::CStr::from_ptr(fdsp_jit_compiler()) }.to_string_lossy().into_owned()
    }

    /// Tolerance mode (FDSP_MATH_FAST): FMA polynomials for feed-forward transcendentals, recurrences exact.
    pub fn set_fast_math(&mut self, on: bool) -> Result<(), String> {
        let c = CString::new("math").unwrap();
        check(unsafe { fdsp_bank_set_option(self.bank, c.as_ptr(), if on { FDSP_MATH_FAST } else { FDSP_MATH_EXACT }) })
    }

    /// Raw handle for device-resident rendering (`fdsp_bank_process`, `fdsp_mix_stereo`, `fdsp_mix_allreduce`).
    pub fn raw(&mut self) -> *mut FdspBank { self.bank }

    /// The big-block entry (the reference's `BigBlockAdapter::process_big`, src/audiounit.rs:510-528, without the 64-sample
    /// chopping: the kernel blocks internally exactly like `Wave::render`).  Device-resident I/O, voice-minor:
    /// `input` = `[inputs][frames][voices]`, `output` = `[outputs][frames][voices]` f32 in HBM; `stream` = a `hipStream_t` or null
    /// (the bank's own stream).  Asynchronous: [`Self::synchronize`] or the caller's stream order the read-back.
    /// This -- not `process()` -- is the throughput path: `process()` follows `AudioNode`'s contract on HOST buffers and moves
    /// `voices x (inputs + outputs) x 256 B` over PCIe per 64-frame block (16.7 MB per block at 65 536 mono voices).
    pub fn render_device(&mut self, frames: usize, input: DevicePtr<'_>, output: DevicePtrMut<'_>, stream: *mut c_void) -> Result<(), String> {
        let (i, o) = unsafe { (fdsp_bank_inputs(self.bank) as usize, fdsp_bank_outputs(self.bank) as usize) };
        if input.len < i * frames * self.voices || output.len < o * frames * self.voices {
            return Err(format!("render_device: buffers of {} / {} floats, the launch needs {} / {}", input.len, output.len,
                               i * frames * self.voices, o * frames * self.voices));
        }
        check(unsafe { fdsp_bank_process(self.bank, frames, input.ptr, output.ptr, FDSP_LAYOUT_VOICE_MINOR, 0, FDSP_MODE_PROCESS, stream) })
    }

    /// Render AND mix down in one launch (`fdsp_bank_process_mix`): what `voice >> pan(p)` per voice followed by the sum over
    /// the voices computes (src/pan.rs:50-76, src/audionode.rs:2406-2462), without the per-voice output ever existing in HBM.
    /// `pan = true`: mono graphs, every voice panned with its own position ([`Self::set_pan`]); `mix` = `[2][frames]`.
    /// `pan = false`: the sum of every output channel over the voices; `mix` = `[outputs][frames]`.
    /// Fixed summation order (include/fundsp_hip.h): bit-identical from launch to launch and across launch geometries.
    pub fn render_mix(&mut self, frames: usize, input: DevicePtr<'_>, mix: DevicePtrMut<'_>, pan: bool, stream: *mut c_void) -> Result<(), String> {
        let (i, o) = unsafe { (fdsp_bank_inputs(self.bank) as usize, fdsp_bank_outputs(self.bank) as usize) };
        let nm = if pan { 2 } else { o };
        if input.len < i * frames * self.voices || mix.len < nm * frames {
            return Err(format!("render_mix: buffers of {} / {} floats, the launch needs {} / {}", input.len, mix.len, i * frames * self.voices, nm * frames));
        }
        check(unsafe { fdsp_bank_process_mix(self.bank, frames, input.ptr, mix.ptr, if pan { FDSP_MIX_PAN } else { FDSP_MIX_SUM }, FDSP_MODE_PROCESS, stream) })
    }

    /// [`Self::render_mix`] of an effect bank (reverbs, networks) from a PLANAR input `[instances][inputs][frame_stride]`, the layout
    /// their kernels read (`fdsp_bank_process_mix_planar`); the same mix bits as the voice-minor call.  Voice banks answer an error.
    pub fn render_mix_planar(&mut self, frames: usize, input: DevicePtr<'_>, frame_stride: usize, mix: DevicePtrMut<'_>, pan: bool,
                             stream: *mut c_void) -> Result<(), String> {
        let (i, o) = unsafe { (fdsp_bank_inputs(self.bank) as usize, fdsp_bank_outputs(self.bank) as usize) };
        let nm = if pan { 2 } else { o };
        if frame_stride < frames || input.len < self.voices * i * frame_stride || mix.len < nm * frames {
            return Err(format!("render_mix_planar: buffers of {} / {} floats, the launch needs {} / {}", input.len, mix.len, self.voices * i * frame_stride, nm * frames));
        }
        check(unsafe { fdsp_bank_process_mix_planar(self.bank, frames, input.ptr, frame_stride, mix.ptr, if pan { FDSP_MIX_PAN } else { FDSP_MIX_SUM }, FDSP_MODE_PROCESS, stream) })
    }

    /// Pan position (-1 .. 1) per voice for `render_mix(.., pan = true, ..)`; every voice starts in the centre (`pan(0.0)`).
    pub fn set_pan(&mut self, pan: &[f32]) -> Result<(), String> {
        check(unsafe { fdsp_bank_set_pan(self.bank, pan.as_ptr(), 0, pan.len()) })
    }

    /// A score for the pool of voices (`Sequencer::push` once per note, `include/fundsp_hip.h` "scores"): note `k` plays on `voice[k]` from
    /// `events[k] = [start, end, fade_in, fade_out]` (seconds) as a fresh unit with the voice's hash and parameters and `params[k * names.len() ..]`
    /// written over the f32 slots `names`.  `fade`: `FDSP_FADE_POWER` / `FDSP_FADE_SMOOTH` per note, or empty for smooth.  `render_events_mix`
    /// (`fdsp_bank_process_events_mix`) then plays it; an empty score removes it.
    pub fn set_score(&mut self, voice: &[i32], events: &[[f64; 4]], fade: &[i32], names: &[&str], params: &[f32]) -> Result<(), String> {
        if events.len() != voice.len() || (!fade.is_empty() && fade.len() != voice.len()) || params.len() != voice.len() * names.len() {
            return Err("set_score: voice, events, fade and params must describe the same notes".into());
        }
        let names: Vec<CString> = names.iter().map(|n| CString::new(*n).map_err(|e| e.to_string())).collect::<Result<_, _>>()?;
        let ptrs: Vec<*const c_char> = names.iter().map(|n| n.as_ptr()).collect();
        check(unsafe {
            fdsp_bank_set_score(self.bank, voice.len(), voice.as_ptr(), events.as_ptr() as *const f64, if fade.is_empty() { core::ptr::null() } else { fade.as_ptr() },
                                ptrs.len() as c_int, ptrs.as_ptr(), params.as_ptr())
        })
    }

    /// `AudioNode::allocate` for the mix path: size the bank's partial-mix buffer for launches of up to `frames` frames, so that
    /// `render_mix` never allocates (real-time loops, HIP graph capture).
    pub fn allocate_mix(&mut self, frames: usize) -> Result<(), String> { check(unsafe { fdsp_bank_mix_reserve(self.bank, frames) }) }

    /// Wait for the bank's own stream (renders launched with a null `stream`).
    pub fn synchronize(&mut self) -> Result<(), String> { check(unsafe { fdsp_bank_synchronize(self.bank) }) }
}

/// A borrowed run of f32 in DEVICE memory (hipMalloc'd by the host application): pointer + length in floats.  The shim never
/// dereferences it on the host; the length is what the launch-size check needs.  A generator's input is `DevicePtr::null()`.
#[derive(Clone, Copy)]
pub struct DevicePtr<'a> { ptr: *const f32, len: usize, _life: PhantomData<&'a f32> }
pub struct DevicePtrMut<'a> { ptr: *mut f32, len: usize, _life: PhantomData<&'a mut f32> }
impl<'a> DevicePtr<'a> {
    /// # Safety
    /// `ptr` must be device memory of at least `len` floats on the bank's device, alive for `'a` and not written while a launch reads it.
    pub unsafe fn new(ptr: *const f32, len: usize) -> Self { Self { ptr, len, _life: PhantomData } }
    pub fn null() -> Self { Self { ptr: core::ptr::null(), len: 0, _life: PhantomData } }
}
impl<'a> DevicePtrMut<'a> {
    /// # Safety
    /// `ptr` must be device memory of at least `len` floats on the bank's device, alive for `'a`, with no other reader or writer while a launch runs.
    pub unsafe fn new(ptr: *mut f32, len: usize) -> Self { Self { ptr, len, _life: PhantomData } }
}

impl<NI: Size<f32>, NO: Size<f32>> AudioNode for HipBank<NI, NO> {
    const ID: u64 = 0x4849_5042; // "HIPB"
    type Inputs = NI;
    type Outputs = NO;

    fn reset(&mut self) {
        // infallible in FunDSP (src/audionode.rs:52); a failed device call is kept for take_error()
        if unsafe { fdsp_bank_reset(self.bank) } != FDSP_OK {
            self.last_error = Some(last_error());
        }
    }

    fn set_sample_rate(&mut self, sample_rate: f64) {
        let rc = unsafe { fdsp_bank_set_sample_rate(self.bank, sample_rate) };
        debug_assert!(rc == FDSP_OK, "{}", last_error());
    }

    #[inline]
    fn tick(&mut self, input: &Frame<f32, Self::Inputs>) -> Frame<f32, Self::Outputs> {
        // one sample of every voice: planar rows of length 1 are [voice][channel] = the Frame's own order
        let mut out: Frame<f32, Self::Outputs> = Frame::default();
        if !self.arity_ok() {
            self.last_error = Some("tick: the bank was created with new_unchecked_arity; drive it through render_device / render_mix".into());
            return out;
        }
        let inp = if NI::USIZE > 0 { input.as_slice().as_ptr() } else { core::ptr::null() };
        let rc = unsafe { fdsp_bank_process_host(self.bank, 1, inp, out.as_mut_slice().as_mut_ptr(), FDSP_LAYOUT_PLANAR, 1, FDSP_MODE_TICK) };
        if rc != FDSP_OK {
            self.last_error = Some(last_error());
            out = Frame::default(); // silence, not stale samples
            debug_assert!(false, "{}", last_error());
        }
        out
    }

    fn process(&mut self, size: usize, input: &BufferRef, output: &mut BufferMut) {
        // BufferRef(&[F32x]) / BufferMut(&mut [F32x]): contiguous [channel][64] f32, 32-byte aligned, channel = voice-major
        if !self.arity_ok() {
            self.last_error = Some("process: the bank was created with new_unchecked_arity; drive it through render_device / render_mix".into());
            for ch in 0..NO::USIZE {
                output.channel_f32_mut(ch)[..size].fill(0.0);
            }
            return;
        }
        let inp = if NI::USIZE > 0 { input.channel_f32(0).as_ptr() } else { core::ptr::null() };
        let out = output.channel_f32_mut(0).as_mut_ptr();
        let rc = unsafe { fdsp_bank_process_host(self.bank, size, inp, out, FDSP_LAYOUT_PLANAR, MAX_BUFFER_SIZE, FDSP_MODE_PROCESS) };
        // process() is infallible in FunDSP: an error here is a programming error (wrong arity, lost device).  The block is
        // silenced (never left holding stale samples) and the error kept for take_error(), in release builds too.
        if rc != FDSP_OK {
            self.last_error = Some(last_error());
            for ch in 0..NO::USIZE {
                output.channel_f32_mut(ch)[..size].fill(0.0);
            }
            debug_assert!(false, "{}", last_error());
        }
    }

    fn set_hash(&mut self, hash: u64) {
        // ping() reaches a leaf with ONE hash; a bank is V leaves: every voice gets it (a bank that should de-correlate
        // its voices calls set_seeds with one seed per voice instead, as the parity tests do)
        let seeds = vec![hash; self.voices];
        if unsafe { fdsp_bank_set_seed(self.bank, seeds.as_ptr(), 0, self.voices) } != FDSP_OK {
            self.last_error = Some(last_error()); // set_hash is infallible (src/audionode.rs:136): kept for take_error()
        }
    }

    fn route(&mut self, input: &SignalFrame, _frequency: f64) -> SignalFrame {
        Routing::Arbitrary(0.0).route(input, self.outputs())
    }
}

impl<NI: Size<f32>, NO: Size<f32>> Clone for HipBank<NI, NO> {
    /// FunDSP nodes are `Clone` (Net and Sequencer clone their units): a second bank that continues exactly where this one
    /// stands.  `fdsp_bank_clone` copies everything a later `set_param` / `reset` / `process` depends on -- the slots, the
    /// delay rings, the SAMPLE RATE and the arithmetic mode (a clone rebuilt from the slot words alone would re-derive its
    /// coefficients at the 44.1 kHz default on the next parameter change), launch options, scheduler events and clock.
    /// `Clone::clone` cannot fail, so a failed copy (device lost, out of memory) panics with the engine's message.
    fn clone(&self) -> Self {
        let mut bank: *mut FdspBank = core::ptr::null_mut();
        let rc = unsafe { fdsp_bank_clone(self.bank, &mut bank) };
        assert!(rc == FDSP_OK && !bank.is_null(), "fdsp_bank_clone: {}", last_error());
        Self { bank, kind: self.kind.clone(), voices: self.voices, ring_frames: self.ring_frames, device: self.device,
               last_error: None, convolve_terms: self.convolve_terms, _marker: PhantomData }
    }
}

impl<NI: Size<f32>, NO: Size<f32>> Drop for HipBank<NI, NO> {
    fn drop(&mut self) {
        unsafe { fdsp_bank_destroy(self.bank) }
    }
}
