// stft_host.hpp — what the host side of the STFT libraries (stft, istft, stftn, istftn, spec) does the same way on top of
// host_plumbing.hpp: the refusals of a geometry, a shape and a stride, the plan-create sequence, the window, the checks an execution
// makes before it launches, the grid of the overlap-add and, for the libraries of the short frame lengths, the tables of csrc/k256r.hpp.
//
// The frame length n is a run-time argument everywhere: the 4096 pair passes 4096 and std::to_string(n) spells the messages. A
// forward plan reads signals and writes frames, an inverse plan reads frames and writes signals; stft_rules says which, and the
// stride check and the plan-create sequence serve both ways round.
//
// Header only, everything in an unnamed namespace, as host_plumbing.hpp: one translation unit and one error string per library,
// nothing linked. The templates take any plan struct that has the fields they name.
#pragma once

#include "host_plumbing.hpp"

// A short-frame library defines STFT_HOST_256R as the namespace of its restatement of csrc/k256r.hpp (stft256r / istft256r) before
// it includes this header.
//
// csrc/k256r.hpp for the host pass alone: build_tables, and what the restatement says of it, held to the original below. In the
// device pass the header would add stockham::copy_kernel, which is no template, to the library's code object; that pass parses
// the host code too, so what it calls is declared for both.
#ifdef STFT_HOST_256R
namespace k256r_host {
void build_tables(int R, std::vector<uint8_t>& blob);       // k256r::build_tables(R, blob): sequential scaling, the default plan's
}
#if !defined(__HIP_DEVICE_COMPILE__)
#include "../csrc/k256r.hpp"

void k256r_host::build_tables(int R, std::vector<uint8_t>& blob) { k256r::build_tables(R, blob); }

#define STFT_HOST_STR_(x) #x
#define STFT_HOST_STR(x) STFT_HOST_STR_(x)
static_assert(STFT_HOST_256R::kDataBytes == k256r::kDataBytes && STFT_HOST_256R::kOffFa == k256r::kOffFa &&
                  STFT_HOST_256R::kOffFb == k256r::kOffFb && STFT_HOST_256R::kOffS == k256r::kOffS,
              STFT_HOST_STR(STFT_HOST_256R) ".hpp and csrc/k256r.hpp disagree on the table blob");
template <int R>
constexpr bool same_layout() {
  for (int n1 = 0; n1 < 16; ++n1)
    if (STFT_HOST_256R::swz(R, n1) != k256r::swz(R, n1)) return false;
  return STFT_HOST_256R::table_bytes<R>() == k256r::table_bytes<R>() && STFT_HOST_256R::lds_bytes<R>() == k256r::lds_bytes<R>();
}
static_assert(same_layout<2>() && same_layout<4>() && same_layout<8>(),
              STFT_HOST_STR(STFT_HOST_256R) ".hpp and csrc/k256r.hpp disagree on the LDS image");
#endif
#endif

namespace {

constexpr uint64_t kMaxExtent = uint64_t{1} << 62;       // halves: a byte offset then fits 64 bits

constexpr uint64_t bins_of(uint64_t n) { return n / 2 + 1; }
constexpr uint64_t pitch_of(uint64_t n) { return (bins_of(n) + 7) & ~uint64_t{7}; }      // tfft_rplan_spectrum_pitch(n)
// (count - 1) * stride + len below `limit` elements (2^62 halves), without overflow
inline bool extent_fits(uint64_t count, uint64_t stride, uint64_t len, uint64_t limit = kMaxExtent) {
  return count == 1 || stride <= (limit - len - 1) / (count - 1);
}

// The frame side of a plan whose frames are not [RE | IM] planes of n / 2 + 1 halves (the spectrogram plans write fp32): what a
// frame holds, the default stride, what a stride must be a multiple of (1: anything), and the unit with its size in bytes
struct frame_layout {
  uint64_t len, dflt, multiple, elem_bytes;
  const char* unit;                  // "floats"
};

// what differs between the four libraries in what they refuse and how they say it
struct stft_rules {
  const char* name;                  // "istftn": libtfft_istftn.so, tfft_istftn_opts, tfft_istftn_plan_set_window
  bool inverse;                      // the frames are the input and the signals the output
  int flag_mask;                     // the flag bits a plan takes
  const char* flags_rule;            // how the message states that, after "<opts name>.flags "
  int (*check_n)(uint32_t);          // the frame lengths of a short-frame library; null where 4096 is the only one
};

// the frames per signal; `frames` may be null
inline int check_geometry(uint64_t n, uint64_t length, uint64_t hop, uint64_t pad, uint64_t* frames) {
  if (length < 8 || length % 8) return fail(TFFT_ERR_ARG, "length must be a multiple of 8 and at least 8");
  if (length > kMaxLength) return fail(TFFT_ERR_ARG, "length must not exceed 2^26");
  if (hop < 8 || hop % 8) return fail(TFFT_ERR_ARG, "hop must be a multiple of 8 and at least 8");
  if (pad % 8 || pad >= n) return fail(TFFT_ERR_ARG, "pad must be a multiple of 8 and below " + std::to_string(n));
  if (length + 2 * pad < n) return fail(TFFT_ERR_ARG, "length + 2 * pad must be at least " + std::to_string(n) + ": there is no frame");
  if (frames) *frames = 1 + (length + 2 * pad - n) / hop;
  return TFFT_OK;
}

inline int check_shape(const stft_rules& rules, uint64_t n, uint64_t rows, uint64_t length, uint64_t hop, uint64_t pad, int flags, uint64_t* frames) {
  uint64_t f = 0;
  int rc = rules.check_n ? rules.check_n(static_cast<uint32_t>(n)) : TFFT_OK;
  if (rc == TFFT_OK) rc = check_geometry(n, length, hop, pad, &f);
  if (rc) return rc;
  if (flags & ~rules.flag_mask)
    return fail(TFFT_ERR_ARG, "unknown flag bits (" + std::to_string(flags) + "): tfft_" + rules.name + "_opts.flags " + rules.flags_rule);
  if (rows == 0 || rows > 0xffffffffull) return fail(TFFT_ERR_ARG, "rows must be in [1, 2^32)");
  // frames < 2^24 (length <= 2^26, pad < n <= 4096, hop >= 8): the product cannot overflow 64 bits. The index 2 i + 1 of the second
  // frame of a pair must fit 32 bits
  if (rows * f > 0xffffffffull) return fail(TFFT_ERR_ARG, "the frame count rows * frames must be below 2^32");
  if (frames) *frames = f;
  return TFFT_OK;
}

// The strides of the two sides, 0 for the default: `sig_field` / `frame_field` as the options struct names them ("in_sig_stride" /
// "out_frame_stride", or "out_sig_stride" / "in_frame_stride" with `frames_in`). The input side is looked at first
// A frame side of another kind comes as `layout`: its extent stays below 2^63 bytes as that of halves does
inline int check_strides(uint64_t n, uint64_t rows, uint64_t length, uint64_t frames, const char* sig_field, uint64_t sig_stride,
                         const char* frame_field, uint64_t frame_stride, bool frames_in, const frame_layout* layout = nullptr) {
  struct side {
    const char* field;
    const char* count;
    uint64_t stride, dflt, blocks, len;
    std::string len_text;
    uint64_t multiple, limit;
    std::string limit_text;
  };
  const side sig = {sig_field, "rows", sig_stride, length, rows, length, "length", 8, kMaxExtent, "2^62 halves"};
  const side frm = layout ? side{frame_field, "rows * frames", frame_stride, layout->dflt, rows * frames, layout->len, std::to_string(layout->len),
                                 layout->multiple, 2 * kMaxExtent / layout->elem_bytes,
                                 "2^" + std::to_string(layout->elem_bytes == 4 ? 61 : 62) + " " + layout->unit}
                          : side{frame_field, "rows * frames", frame_stride, 2 * pitch_of(n), rows * frames, bins_of(n), std::to_string(bins_of(n)), 8,
                                 kMaxExtent, "2^62 halves"};
  const side* const in_out[2] = {frames_in ? &frm : &sig, frames_in ? &sig : &frm};
  for (const side* s : in_out)
    if (s->stride && (s->stride % s->multiple || s->stride < s->len))
      return fail(TFFT_ERR_ARG, std::string(s->field) + " must be 0 or " +
                                    (s->multiple > 1 ? "a multiple of " + std::to_string(s->multiple) + " that is >= " : ">= ") + s->len_text);
  for (int i = 0; i < 2; ++i) {
    const side* s = in_out[i];
    if (!extent_fits(s->blocks, s->stride ? s->stride : s->dflt, s->len, s->limit))
      return fail(TFFT_ERR_ARG, std::string("the ") + (i ? "output" : "input") + " extent (" + s->count + " - 1) * " + s->field + " + " + s->len_text +
                                    " must be below " + s->limit_text);
  }
  return TFFT_OK;
}

// ---- a plan. Plan has: n, rows, length, hop, pad, frames, total (= rows * frames), in_stride, out_stride, launch_iters, device,
// num_cus, d_tables, d_window (n halves, the plan's own copy), have_window.
//
// The plan-create sequence of all four. `o` holds the defaults on entry; `sig` / `frm` are the signal and the frame stride of Opts.
// `finish(p, o)` runs on the plan's device: it fills what is the library's own and creates the device state. A library whose
// frames are no planes of halves passes `frame_side(n, o, layout)`: it refuses what is wrong with the options of its own, after the
// shape and before the strides, and states the layout of a frame
template <class Plan, class Opts, class Finish>
int create_plan(const stft_rules& rules, uint64_t n, uint64_t rows, uint64_t length, uint64_t hop, uint64_t pad, int device_id, const Opts* opts, Opts o,
                uint64_t Opts::*sig, uint64_t Opts::*frm, Plan** out, void (*destroy)(Plan*), Finish finish,
                int (*frame_side)(uint64_t, const Opts&, frame_layout&) = nullptr) {
  g_err.clear();
  if (!out) return fail(TFFT_ERR_ARG, "null plan pointer");
  *out = nullptr;
  const std::string name = std::string("tfft_") + rules.name;
  int rc = take_opts(opts, (name + "_opts").c_str(), o);
  if (rc) return rc;
  uint64_t frames = 0;
  frame_layout layout = {};
  rc = check_shape(rules, n, rows, length, hop, pad, o.flags, &frames);
  if (rc == TFFT_OK && frame_side) rc = frame_side(n, o, layout);
  if (rc == TFFT_OK)
    rc = rules.inverse ? check_strides(n, rows, length, frames, "out_sig_stride", o.*sig, "in_frame_stride", o.*frm, true, frame_side ? &layout : nullptr)
                       : check_strides(n, rows, length, frames, "in_sig_stride", o.*sig, "out_frame_stride", o.*frm, false, frame_side ? &layout : nullptr);
  if (rc == TFFT_OK) rc = check_launch_iters(o.launch_iters);
  if (rc == TFFT_OK) rc = check_abi(("lib" + name + ".so").c_str());
  if (rc == TFFT_OK) rc = pass_tfft(tfft_device_check(device_id));
  if (rc) return rc;
  int prev = 0;
  CONV_HIP(hipGetDevice(&prev));
  CONV_HIP(hipSetDevice(device_id));
  Plan* p = new Plan;
  p->n = n;
  p->rows = rows;
  p->length = length;
  p->hop = hop;
  p->pad = pad;
  p->frames = frames;
  p->total = rows * frames;
  const uint64_t sig_stride = o.*sig ? o.*sig : length, frame_stride = o.*frm ? o.*frm : frame_side ? layout.dflt : 2 * pitch_of(n);
  p->in_stride = rules.inverse ? frame_stride : sig_stride;
  p->out_stride = rules.inverse ? sig_stride : frame_stride;
  p->launch_iters = o.launch_iters;
  p->device = device_id;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) p->num_cus = prop.multiProcessorCount;
  rc = finish(p, o);
  (void)hipSetDevice(prev);
  if (rc) return fail_create(p, rc, destroy);
  *out = p;
  return TFFT_OK;
}

// the device memory every plan has: a copy of the kernel's constant tables, the first `table_bytes` of `blob`, and the window
template <class Plan>
int create_device_base(Plan* p, const std::vector<uint8_t>& blob, size_t table_bytes) {
  CONV_HIP(hipMalloc(&p->d_tables, table_bytes));
  CONV_HIP(hipMemcpy(p->d_tables, blob.data(), table_bytes, hipMemcpyHostToDevice));
  CONV_HIP(hipMalloc(reinterpret_cast<void**>(&p->d_window), p->n * 2));
  return TFFT_OK;
}
template <class Plan>
void destroy_device_base(Plan* p) {
  if (p->d_tables) (void)hipFree(p->d_tables);
  if (p->d_window) (void)hipFree(p->d_window);
}

template <class Plan>
int set_window(Plan* p, const void* window, void* stream) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  if (!window) return fail(TFFT_ERR_ARG, "null window pointer");
  const int rc = check_current(p->device);
  if (rc) return rc;
  CONV_HIP(hipMemcpyAsync(p->d_window, window, p->n * 2, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
  p->have_window = true;
  return TFFT_OK;
}

// ---- what an execution checks before it launches; a, b, c are its three data pointers in the order of the call
template <class Plan>
int check_exec_args(const stft_rules& rules, const Plan* p, const void* a, const void* b, const void* c) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  if (!p->have_window) return fail(TFFT_ERR_ARG, std::string("no window: call tfft_") + rules.name + "_plan_set_window first");
  if (!a || !b || !c) return fail(TFFT_ERR_ARG, "null data pointer");
  if ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15)
    return fail(TFFT_ERR_ARG, "data pointers must be 16-byte aligned");
  return TFFT_OK;
}

template <class Plan>
int check_exec_forward(const stft_rules& rules, const Plan* p, const void* in, void* out_re, void* out_im) {
  const int rc = check_exec_args(rules, p, in, out_re, out_im);
  if (rc) return rc;
  // frames of one signal overlap, and frames are work items of different waves that run in no defined order: the input's extent
  // (gaps included) must stay clear of both output planes' extents
  const uint64_t bins = bins_of(p->n);
  const uint64_t in_bytes = 2 * ((p->rows - 1) * p->in_stride + p->length), out_bytes = 2 * ((p->total - 1) * p->out_stride + bins);
  if (blocks_overlap(in, in_bytes, out_re, out_bytes) || blocks_overlap(in, in_bytes, out_im, out_bytes))
    return fail(TFFT_ERR_ARG, "input and output overlap (an STFT plan cannot run in place: frames share input samples)");
  // the two planes may interleave ([RE h | IM h] blocks); their written parts, n / 2 + 1 halves per frame, may not share a half
  if (seqs_overlap(out_re, p->out_stride, bins, out_im, p->out_stride, bins, p->total))
    return fail(TFFT_ERR_ARG, "the RE and IM output planes overlap");
  return check_current(p->device);
}

// Plan has also the workspace fields of host_plumbing.hpp (ws_need: rows * frames * n halves, the time-domain frames); the
// workspace is settled here
template <class Plan>
int check_exec_inverse(const stft_rules& rules, const Plan* p, const void* in_re, const void* in_im, void* out) {
  int rc = check_exec_args(rules, p, in_re, in_im, out);
  if (rc) return rc;
  // whole extents, gaps included (conservative): the inputs are never written, and frames are work items that run in no defined order
  const uint64_t in_bytes = 2 * ((p->total - 1) * p->in_stride + bins_of(p->n)), out_bytes = 2 * ((p->rows - 1) * p->out_stride + p->length);
  if (blocks_overlap(out, out_bytes, in_re, in_bytes) || blocks_overlap(out, out_bytes, in_im, in_bytes))
    return fail(TFFT_ERR_ARG, "output and input overlap (an ISTFT plan cannot run in place)");
  rc = check_current(p->device);
  if (rc == TFFT_OK) rc = ws_ensure(p);
  if (rc) return rc;
  if (blocks_overlap(p->ws, p->ws_need, out, out_bytes)) return fail(TFFT_ERR_ARG, "the workspace overlaps the output");
  if (blocks_overlap(p->ws, p->ws_need, in_re, in_bytes) || blocks_overlap(p->ws, p->ws_need, in_im, in_bytes))
    return fail(TFFT_ERR_ARG, "the workspace overlaps the input");
  return TFFT_OK;
}

// ---- the launch of the overlap-add (istft/ola.hpp, istftn/olan.hpp), one thread per chunk of 8 output samples
// The kernel's frame range is signed 64-bit arithmetic on hop. With more than one frame per signal (F - 1) * hop <= L + 2 pad - n
// < 2^27; a plan with ONE frame may have any hop up to 2^64 - 8, and all the kernel needs of it is that no second frame starts
// inside the padded signal: such a plan passes L + 2 pad, which is what every hop beyond L + 2 pad - n amounts to
template <class Plan>
uint64_t ola_hop(const Plan* p) {
  return p->frames > 1 ? p->hop : p->length + 2 * p->pad;
}
template <class Plan>
uint32_t ola_grid(const Plan* p, uint64_t block) {
  const uint64_t blocks = (p->rows * (p->length / 8) + block - 1) / block;
  return static_cast<uint32_t>(std::min<uint64_t>(blocks, static_cast<uint64_t>(p->num_cus) * 32));
}

}  // namespace
