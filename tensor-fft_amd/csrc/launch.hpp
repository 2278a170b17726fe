// launch.hpp - the launch layer of tfft.hip: how a plan becomes kernel launches. Included into tfft.hip's unnamed namespace behind
// tfft_plan and plan_passes, the way dist.hpp, staging.hpp and rfft.hpp are included behind the C ABI. From top to bottom: the LDS
// opt-in, the Launch context and the one launch() function, the grid shape helpers, the per-kernel launchers, the column dispatch
// table, launch_chain, acquire_workspace and the walks (prepare_kernels, record_kernels).

// Opt-in to more than 64 KiB of dynamic LDS, once per (kernel, device). The outcome is STICKY: a failure is returned on
// every later call too (a std::call_once would report it once and then launch without the attribute). Plans run this
// for every kernel they can launch at creation time (the OptIn walk below), so tfft_exec stays a pure launch, also under
// stream capture; the call here then only finds its map entry.
int lds_opt_in(const void* fn, int device, int bytes) {
  static std::mutex m;
  static std::map<std::pair<const void*, int>, hipError_t> done;
  hipError_t e;
  {
    std::lock_guard<std::mutex> lock(m);
    const auto key = std::make_pair(fn, device);
    auto it = done.find(key);
    if (it == done.end()) it = done.emplace(key, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes)).first;
    e = it->second;
  }
  if (e != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(MaxDynamicSharedMemorySize)");
  return TFFT_OK;
}
// Column slab of a four-step radix-256 pass (dist.hpp: the exchange of a distributed transform overlapped slab by slab): filled by
// dist_launch_col for one launch_chain call, read by launch_col. Columns, not blocks: the block width is chosen at the launch site.
struct SlabCtx {
  uint64_t col_first = 0, col_count = 0;
  uint32_t out_pitch_shift = 0, out_seg_shift = 31;
  uint64_t out_seg_gap = 0, out_base = 0;
};
// The launch logic of a plan runs in three ways, and every function of the launch layer takes the way as its first argument:
//   Run     an execution: LDS opt-in (a map look-up after plan creation), then the launch, on `stream`
//   OptIn   at plan creation: lds_opt_in for every kernel an execution would select; nothing is launched or allocated
//   Record  tfft_plan_kernels & co.: the name of every kernel an execution would launch is appended to `names`; no runtime call
//           besides the symbol look-up, nothing is launched or allocated
// The two walks run over stand-in pointers (walk_ptrs, kFakeWorkspace). The context is the caller's local: nothing of it outlives
// the call, and nothing another thread does can reach it.
enum class Mode { Run, OptIn, Record };
struct Recorder {
  std::vector<std::string>* names;               // the kernels in launch order ...
  std::string mismatch;                          // ... and the first site whose name is not its function's
};
struct Launch {
  Mode mode;
  hipStream_t stream;
  Recorder* rec;                                 // Record only
  const SlabCtx* slab;                           // column slab of a distributed transform, or none
  static Launch run(void* stream) { return Launch{Mode::Run, static_cast<hipStream_t>(stream), nullptr, nullptr}; }
  static Launch opt_in() { return Launch{Mode::OptIn, nullptr, nullptr, nullptr}; }
  static Launch record(Recorder& rec) { return Launch{Mode::Record, nullptr, &rec, nullptr}; }
};
// Stand-ins for the data pointers and the workspace of a walk: never dereferenced, only kept apart from each other, so that every pass
// sees the pointer relations of an execution. Four planes `span` bytes apart (0: the one address, for a launcher that only selects its
// kernel), or the [RE | IM] block of an in-place execution with planes `plane` bytes apart.
_Float16* const kFakeWorkspace = reinterpret_cast<_Float16*>(uintptr_t{1} << 46);
struct WalkPtrs {
  uint8_t *in_re, *in_im, *out_re, *out_im;
};
inline WalkPtrs walk_ptrs(uint64_t span) {
  uint8_t* const base = reinterpret_cast<uint8_t*>(uintptr_t{1} << 20);
  return WalkPtrs{base, base + span, base + 2 * span, base + 3 * span};
}
inline WalkPtrs walk_ptrs_in_place(uint64_t plane) {
  const WalkPtrs f = walk_ptrs(plane);
  return WalkPtrs{f.in_re, f.in_im, f.in_re, f.in_im};
}
// Kernel names as c++filt prints the code object's symbol without its parameter list (the names of tfft_kernel_list): written at the
// launch site as kname("ns::kernel", template arguments ...) and only put together while recording (that allocates). The recorder
// checks the name against the runtime's symbol of the function pointer launched there (hipKernelNameRefByPtr, demangled), so a name
// can only be listed for the kernel it names.
inline std::string targ(bool b) { return b ? "true" : "false"; }
inline std::string targ(int v) { return std::to_string(v); }
template <class... A>
auto kname(const char* base, A... args) {
  return [=] {
    std::string s = base;
    const char* sep = "<";
    ((s += sep, s += targ(args), sep = ", "), ...);
    return sizeof...(A) ? s + ">" : s;
  };
}
inline void note_kernel(Recorder& rec, const void* fn, const std::string& name) {
  const char* sym = hipKernelNameRefByPtr(fn, nullptr);
  int status = -1;
  char* dem = sym ? abi::__cxa_demangle(sym, nullptr, nullptr, &status) : nullptr;
  std::string d = dem ? dem : (sym ? sym : "(no symbol)");
  std::free(dem);
  if (d.compare(0, 5, "void ") == 0) d.erase(0, 5);
  d = d.substr(0, d.find('('));
  if (d != name && rec.mismatch.empty()) rec.mismatch = name + " at the launch site of " + d;
  rec.names->push_back(name);
}
// The one launch site of the launch layer. LDS opt-in exactly where a kernel takes dynamic LDS (lds_opt_in is a runtime call once per
// (kernel, device); the OptIn walk at plan creation has made it for every kernel an out-of-place execution selects).
template <class... P, class Name, class... A>
int launch(const Launch& L, int device, void (*kernel)(P...), const Name& name, dim3 grid, dim3 block, uint32_t lds, const A&... args) {
  if (L.mode == Mode::Record) {
    note_kernel(*L.rec, reinterpret_cast<const void*>(kernel), name());
    return TFFT_OK;
  }
  if (lds) {
    const int rc = lds_opt_in(reinterpret_cast<const void*>(kernel), device, static_cast<int>(lds));
    if (rc) return rc;
  }
  if (L.mode == Mode::Run) hipLaunchKernelGGL(kernel, grid, block, lds, L.stream, args...);
  return TFFT_OK;
}

// Grid of a grid-stride ("persistent") kernel whose workgroups each own `iters` work items per wave slot: at least one
// workgroup per CU's worth when there is that much work, otherwise blocks_needed / iters so that the hardware
// dispatcher hands out workgroups as CUs drain (keeps CUs out of lock-step; see launch_k4096_v).
// (launch-shape experiment knobs: environment variables in the debug build only; the shipped library takes its launch
// shapes from the plan, see tfft_plan_opts.launch_iters)
inline uint32_t env_iters(const char* name, uint32_t dflt) {
#ifdef TFFT_DEBUG_KERNELS
  const char* e = std::getenv(name);
  return e ? static_cast<uint32_t>(std::max(0, std::atoi(e))) : dflt;
#else
  (void)name;
  return dflt;
#endif
}
// tfft_plan_opts.launch_iters -> rounds per workgroup: 0 keeps the kernel's measured default, TFFT_LAUNCH_PERSISTENT one
// workgroup per CU for the whole batch
inline uint32_t plan_iters(uint32_t launch_iters, uint32_t dflt) {
  if (launch_iters == 0) return dflt;
  return launch_iters >= TFFT_LAUNCH_PERSISTENT ? 1000000u : launch_iters;
}
inline uint32_t pick_grid(uint64_t blocks_needed, int num_cus, uint32_t iters) {
  const uint64_t lo = std::min<uint64_t>(blocks_needed, static_cast<uint64_t>(num_cus));
  return static_cast<uint32_t>(std::max<uint64_t>(lo, (blocks_needed + iters - 1) / std::max(iters, 1u)));
}

// Grid of the kernels that used to run as persistent workgroups (column passes, k4096r, the fused 2D row pass). Round 4: a
// static partition (one workgroup per CU for the whole batch) ends when the SLOWEST CU ends, and on some boxes CUs differ by
// several per cent; `gens` generations of workgroups, handed out by the hardware dispatcher as CUs drain, balance
// that dynamically. What it buys depends on the box (three boxes, profiles/r4_iters_scan.txt, r4_gens_scan.txt): 2^16 x 16384
// (4-wave radix-256 workgroups, 8 generations) +2.6 %, +2.6 %, +6.5 %; the 8-wave radix-256 / 512 / 1024 kernels with 2 generations
// 0 ... +0.5 % on two boxes and +3.6 ... +5 % on the third (2^20 x 1024: 329 -> 341 Gsamples/s); more generations lose again (tables
// and pipeline fill are paid per workgroup: 2^20 at 8 generations -3 %). The fused 2D row pass and the 8192 ... 32768 kernels
// (one iteration = 13 us) keep the static partition (-1 ... -3 % with two generations). Whole multiples of the resident capacity
// only (a grid of 2.7 capacities leaves a third of the chip idle in its last round: 301 Gsamples/s), and only while every
// workgroup still gets kMinRounds rounds. tfft_plan_opts.launch_iters overrides (the tuner's knob; TFFT_LAUNCH_PERSISTENT = the
// static partition).
inline uint32_t gens_grid(uint64_t blocks, uint32_t capacity, uint32_t launch_iters, uint32_t gens_dflt) {
  if (launch_iters) return pick_grid(blocks, static_cast<int>(capacity), plan_iters(launch_iters, 1000000u));
  static const uint32_t gens_env = env_iters("TFFT_GENS", 0);            // experiment knob (debug build only)
  const uint32_t gens = gens_env ? gens_env : gens_dflt;
  static const uint64_t kMinRounds = env_iters("TFFT_GENS_MIN_ROUNDS", 8);     // (experiment knob in the debug build; 8 otherwise)
  if (gens > 1 && blocks >= static_cast<uint64_t>(capacity) * gens * kMinRounds) return capacity * gens;
  return static_cast<uint32_t>(std::min<uint64_t>(blocks, capacity));
}
constexpr uint32_t kGensStatic = 1, kGensCol8 = 2;    // per kernel family, see above (the radix-256 workgroup kernel: rounds_grid below)

// The radix-256 workgroup kernel since its tables are fetched behind its first block's copy-in (colfft.hpp, end of round 4): a
// workgroup's start-up is cheap enough for about FOUR rounds per workgroup to be the best shape, however many generations that
// makes (profiles/r4_gens_after_prologue.txt, one process: 2^16 x 4096 345 -> 369 Gsamples/s, 2^16 x 16384 357 -> 365, 256-point
// transforms along a strided axis +1 ... +1.5 %; one or two rounds per workgroup lose 1 ... 9 %). Whole multiples of the resident
// capacity, as above.
inline uint32_t rounds_grid(uint64_t blocks, uint32_t capacity, uint32_t launch_iters) {
  if (launch_iters) return pick_grid(blocks, static_cast<int>(capacity), plan_iters(launch_iters, 1000000u));
  constexpr uint64_t kRounds = 4, kMaxGens = 64;
  const uint64_t gens = std::min<uint64_t>(kMaxGens, blocks / (static_cast<uint64_t>(capacity) * kRounds));
  if (gens >= 2) return static_cast<uint32_t>(capacity * gens);
  return static_cast<uint32_t>(std::min<uint64_t>(blocks, capacity));
}

// Waves per workgroup that take work in the single-pass kernels (one transform, or one group of transforms, per wave): 8 when the
// batch fills the chip; for `units` wave-tasks that do not, the fewest (1, 2, 4) that still fit one workgroup per CU, so that the
// tasks spread over the CUs with one wave per SIMD instead of filling a few CUs with two (profiles/r5_small_scan.txt, last part).
// TFFT_VARIANT_PACKED keeps the packed shape (A/B).
inline uint32_t live_waves(const tfft_plan* p, uint64_t units) {
  if (p->variant & TFFT_VARIANT_PACKED) return 8;
  const uint64_t cus = static_cast<uint64_t>(p->num_cus);
  for (uint32_t live = 1; live <= 4; live *= 2)
    if (units <= cus * live) return live;
  return 8;
}

// Launch shape of the N = 4096 kernel for p->batch transforms: waves per workgroup that take work, and the grid
inline void k4096_shape(const tfft_plan* p, uint32_t& live, uint32_t& grid) {
  live = live_waves(p, p->batch);
  const uint32_t blocks_needed = static_cast<uint32_t>((p->batch + live - 1) / live);
  // Workgroups are sized so that each wave runs about two transforms: the second one's HBM->LDS copy flies under
  // the first one's stores, and the hardware dispatcher hands out the remaining workgroups as CUs drain, which keeps
  // the CUs out of lock-step (measured: 256 persistent workgroups 5.3 TB/s, two transforms per wave 6.1 TB/s, one
  // transform per wave 5.1 TB/s; profiles/r1_k4096_grid_scan.txt).
  static const uint32_t iters_env = env_iters("TFFT_K4096_ITERS", 0);   // experiment knob (debug build only)
  const uint32_t iters = iters_env ? iters_env : plan_iters(p->launch_iters, blocks_needed >= 4u * static_cast<uint32_t>(p->num_cus) ? 2u : 1u);
  grid = pick_grid(blocks_needed, p->num_cus, iters);
}

template <int V>
int launch_k4096_v(const Launch& L, const tfft_plan* p, const void* in_re, const void* in_im, void* out_re, void* out_im,
                   k4096::Addr in_stride, k4096::Addr out_stride) {
  uint32_t live, grid;
  k4096_shape(p, live, grid);
  auto go = [&](auto kernel, auto name) {
    return launch(L, p->device, kernel, name, dim3(grid), dim3(k4096::kThreads), k4096::kLdsBytes,
                  static_cast<const uint16_t*>(in_re), static_cast<const uint16_t*>(in_im),
                  static_cast<uint16_t*>(out_re), static_cast<uint16_t*>(out_im), in_stride, out_stride,
                  static_cast<uint32_t>(p->batch), live, static_cast<const uint8_t*>(p->d_tables), p->otw, k4096::RealOut{});
  };
  if constexpr (V == (k4096::kStageOut | k4096::kNonTemporal)) {
    // row pass of a transposed-input plan (default variant only, create_transposed_in)
    if (p->otw.n_mask) return go(k4096::fft4096_kernel<V, true>, kname("k4096::fft4096_kernel", V, true, false));
  }
  return go(k4096::fft4096_kernel<V, false>, kname("k4096::fft4096_kernel", V, false, false));
}

int launch_k256(const Launch& L, const tfft_plan* p, const void* in_re, const void* in_im, void* out_re, void* out_im,
                k4096::Addr in_stride, k4096::Addr out_stride) {
  const uint64_t groups = (p->batch + k256::kFftsPerWave - 1) / k256::kFftsPerWave;
  const uint32_t live = live_waves(p, groups);
  const uint32_t blocks_needed = static_cast<uint32_t>((groups + live - 1) / live);
  static const uint32_t iters_dflt = env_iters("TFFT_K256_ITERS", 2);
  const uint32_t grid = pick_grid(blocks_needed, p->num_cus, plan_iters(p->launch_iters, iters_dflt));
  auto go = [&](auto kernel, auto name) {
    return launch(L, p->device, kernel, name, dim3(grid), dim3(k4096::kThreads), k256::kLdsBytes,
                  static_cast<const uint16_t*>(in_re), static_cast<const uint16_t*>(in_im),
                  static_cast<uint16_t*>(out_re), static_cast<uint16_t*>(out_im), in_stride, out_stride,
                  static_cast<uint32_t>(p->batch), live, static_cast<const uint8_t*>(p->d_tables), p->otw);
  };
  return p->otw.n_mask ? go(k256::fft256_kernel<true>, kname("k256::fft256_kernel", true))
                       : go(k256::fft256_kernel<false>, kname("k256::fft256_kernel", false));
}

template <int R, bool STG>
int launch_k256r_t(const Launch& L, const tfft_plan* p, const void* in_re, const void* in_im, void* out_re, void* out_im,
                   k4096::Addr in_stride, k4096::Addr out_stride) {
  const uint64_t groups = (p->batch + (16 / R) - 1) / (16 / R);
  const uint32_t live = live_waves(p, groups);
  const uint32_t blocks_needed = static_cast<uint32_t>((groups + live - 1) / live);
  static const uint32_t iters_dflt = env_iters("TFFT_K256_ITERS", 2);
  const uint32_t grid = pick_grid(blocks_needed, p->num_cus, plan_iters(p->launch_iters, iters_dflt));
  auto go = [&](auto kernel, auto name) {
    return launch(L, p->device, kernel, name, dim3(grid), dim3(k4096::kThreads), k256r::lds_bytes<R>(),
                  static_cast<const uint16_t*>(in_re), static_cast<const uint16_t*>(in_im),
                  static_cast<uint16_t*>(out_re), static_cast<uint16_t*>(out_im), in_stride, out_stride,
                  static_cast<uint32_t>(p->batch), live, static_cast<const uint8_t*>(p->d_tables), p->otw);
  };
  if constexpr (STG) {
    // row pass of a transposed-input plan (staged stores only, create_transposed_in)
    if (p->otw.n_mask) return go(k256r::fft256r_kernel<R, true, true>, kname("k256r::fft256r_kernel", R, true, true));
  }
  return go(k256r::fft256r_kernel<R, STG, false>, kname("k256r::fft256r_kernel", R, STG, false));
}

int launch_k256r(const Launch& L, const tfft_plan* p, int radix, const void* in_re, const void* in_im, void* out_re, void* out_im,
                 k4096::Addr in_stride, k4096::Addr out_stride) {
  const bool direct = p->variant & TFFT_VARIANT_UNSTAGED_STORES;   // 8-byte stores straight from registers instead of staged full rows
  switch (radix) {
    case 2:
      return direct ? launch_k256r_t<2, false>(L, p, in_re, in_im, out_re, out_im, in_stride, out_stride)
                    : launch_k256r_t<2, true>(L, p, in_re, in_im, out_re, out_im, in_stride, out_stride);
    case 4:
      return direct ? launch_k256r_t<4, false>(L, p, in_re, in_im, out_re, out_im, in_stride, out_stride)
                    : launch_k256r_t<4, true>(L, p, in_re, in_im, out_re, out_im, in_stride, out_stride);
    default:
      return direct ? launch_k256r_t<8, false>(L, p, in_re, in_im, out_re, out_im, in_stride, out_stride)
                    : launch_k256r_t<8, true>(L, p, in_re, in_im, out_re, out_im, in_stride, out_stride);
  }
}

#ifdef TFFT_DEBUG_KERNELS
// measurement hook of tools/exp_k4096r_phases.py and tools/exp_rows_phases.py: one more kernel argument in the debug build
inline unsigned long long* rows_stamps() {
  if (debug_variants_enabled())
    if (const char* e = std::getenv("TFFT_ROWS_STAMPS_PTR")) return reinterpret_cast<unsigned long long*>(std::strtoull(e, nullptr, 0));
  return nullptr;
}
#endif

template <int R>
int launch_k4096r_t(const Launch& L, const tfft_plan* p, const void* in_re, const void* in_im, void* out_re, void* out_im,
                    k4096::Addr in_stride, k4096::Addr out_stride) {
  // transforms per workgroup iteration: 8 / R, or ONE while that still gives every transform a CU of its own (the R waves of a
  // transform then have the SIMDs to themselves: 2^13 x 4 11.7 -> 7.6 us, 2^14 x 2 12.2 -> 8.5 us)
  const uint64_t cus = static_cast<uint64_t>(p->num_cus);
  const uint32_t per_wg = (p->variant & TFFT_VARIANT_PACKED) ? k4096::kWavesPerBlock / R
                          : (R < 8 && p->batch <= cus)   ? 1u
                          : (R == 2 && p->batch <= 2 * cus) ? 2u      // (four waves: still one per SIMD)
                                                            : k4096::kWavesPerBlock / R;
  const uint32_t blocks_needed = static_cast<uint32_t>((p->batch + per_wg - 1) / per_wg);
  // persistent workgroups: with four workgroup barriers per transform the short-lived launch shape of the 4096
  // kernel does not help here (measured at 2^13: 405 / 425 / 440 / 457 Gsamples/s for 1 / 2 / 4 / all iterations)
  const uint32_t grid = gens_grid(blocks_needed, static_cast<uint32_t>(p->num_cus), p->launch_iters, kGensStatic);
  auto go = [&](auto kernel, auto name) {
    return launch(L, p->device, kernel, name, dim3(grid), dim3(k4096::kThreads), k4096::kLdsBytes,
                  static_cast<const uint16_t*>(in_re), static_cast<const uint16_t*>(in_im),
                  static_cast<uint16_t*>(out_re), static_cast<uint16_t*>(out_im), in_stride, out_stride,
                  static_cast<uint32_t>(p->batch), per_wg, static_cast<const uint8_t*>(p->d_tables), p->otw
#ifdef TFFT_DEBUG_KERNELS
                  , rows_stamps()
#endif
    );
  };
  if constexpr (R == 2) {      // (no transposed layout has N2 = 8192, tfft_plan_transposed_n2: no such instantiation either)
    if (p->otw.n_mask) return fail(TFFT_ERR_ARG, "internal error: transposed-input row pass of 8192 points");
  } else if (p->otw.n_mask) {  // row pass of a transposed-input plan
    return go(k4096r::fft4096r_kernel<R, false, true>, kname("k4096r::fft4096r_kernel", R, false, true));
  }
  return go(k4096r::fft4096r_kernel<R, false, false>, kname("k4096r::fft4096r_kernel", R, false, false));
}

int launch_k4096r(const Launch& L, const tfft_plan* p, int radix, const void* in_re, const void* in_im, void* out_re, void* out_im,
                  k4096::Addr in_stride, k4096::Addr out_stride) {
  switch (radix) {
    case 2: return launch_k4096r_t<2>(L, p, in_re, in_im, out_re, out_im, in_stride, out_stride);
    case 4: return launch_k4096r_t<4>(L, p, in_re, in_im, out_re, out_im, in_stride, out_stride);
    default: return launch_k4096r_t<8>(L, p, in_re, in_im, out_re, out_im, in_stride, out_stride);
  }
}

// first pass of the fused 2D plan: iterations = images * 512 (k4096r.hpp, ROWS); p only lends its device and tables
int launch_rows2d(const Launch& L, const tfft_plan* p, const void* in_re, const void* in_im, void* out_re, void* out_im,
                  uint64_t image_stride, uint32_t iterations) {
  const uint32_t grid = gens_grid(iterations, static_cast<uint32_t>(p->num_cus), 0, kGensStatic);
  const int rc = launch(L, p->device, k4096r::fft4096r_kernel<8, true>, kname("k4096r::fft4096r_kernel", 8, true, false), dim3(grid),
                        dim3(k4096::kThreads), k4096::kLdsBytes,
                        static_cast<const uint16_t*>(in_re), static_cast<const uint16_t*>(in_im),
                        static_cast<uint16_t*>(out_re), static_cast<uint16_t*>(out_im), k4096::Addr{image_stride, image_stride, 0, 0},
                        k4096::Addr{image_stride, image_stride, 0, 0}, iterations, 1u, static_cast<const uint8_t*>(p->d_tables), k4096::OutTw{}
#ifdef TFFT_DEBUG_KERNELS
                        , rows_stamps()
#endif
  );
  if (rc) return rc;
  if (L.mode == Mode::Run) TFFT_HIP(hipGetLastError());
  return TFFT_OK;
}

int launch_k4096(const Launch& L, const tfft_plan* p, const void* in_re, const void* in_im, void* out_re, void* out_im,
                 k4096::Addr in_stride, k4096::Addr out_stride) {
  // opts.variant: 0 = default (staged, coalesced, non-temporal stores: the fastest measured on MI355X);
  // otherwise its k4096 bits are the template argument of fft4096_kernel, with TFFT_VARIANT_K4096_PLAIN = "none of them".
  static_assert(TFFT_VARIANT_K4096_PREFETCH == k4096::kPrefetch && TFFT_VARIANT_K4096_STAGE_OUT == k4096::kStageOut &&
                TFFT_VARIANT_K4096_NONTEMPORAL == k4096::kNonTemporal, "variant bits of the N = 4096 kernel are its template flags");
#ifdef TFFT_DEBUG_KERNELS
  static_assert(kDbgK4096FakeStore == k4096::kFakeStore && kDbgK4096NoCompute == k4096::kNoCompute, "debug bits of the N = 4096 kernel");
#endif
  constexpr int kFlags = TFFT_VARIANT_K4096_PREFETCH | TFFT_VARIANT_K4096_STAGE_OUT | TFFT_VARIANT_K4096_NONTEMPORAL |
                         kDbgK4096FakeStore | kDbgK4096NoCompute;
  const int v = (p->variant & (kFlags | TFFT_VARIANT_K4096_PLAIN)) == 0 ? (k4096::kStageOut | k4096::kNonTemporal) : (p->variant & kFlags);
#define TFFT_V(N) case N: return launch_k4096_v<N>(L, p, in_re, in_im, out_re, out_im, in_stride, out_stride)
  switch (v) {
    TFFT_V(0); TFFT_V(1); TFFT_V(2); TFFT_V(8); TFFT_V(9); TFFT_V(10);
#ifdef TFFT_DEBUG_KERNELS      // timing-only instantiations (WRONG output): fake stores / no compute
    TFFT_V(4); TFFT_V(5); TFFT_V(13); TFFT_V(64); TFFT_V(72); TFFT_V(73);
#endif
    default: return fail(TFFT_ERR_ARG, "unknown kernel variant");
  }
#undef TFFT_V
}

struct Planes {
  _Float16* re;
  _Float16* im;
  uint64_t stride;
};

// ---------------------------------------------------------------------------------------------------------------------
// The column kernels this library ships: ONE list per kernel family. The dispatch table below, the names tfft_kernel_list()
// reports and (through tests/test_isa_lint.py, which compares that list with the symbols of the gfx950 code object) the set of
// instantiations in libtfft.so all come from these lists: a further variant is a further row, not a further branch of a ladder.
// Arguments are written the way the demangler prints them (bools as false / true), because the row's name is built from them.
// ---------------------------------------------------------------------------------------------------------------------
// colfft256_kernel<MODE, TW, STAGE, LUT>: per-wave radix-256 pass (16-column tiles)
#define TFFT_COL_WAVE(X)                                                                                     \
  X(0, 1, false, false) X(0, 1, false, true) X(0, 1, true, false) X(0, 1, true, true) X(0, 0, false, false)  \
  X(0, 0, true, false) X(1, 1, false, false) X(1, 1, false, true) X(1, 1, true, false) X(1, 1, true, true)   \
  X(1, 0, false, false) X(1, 0, true, false)
// colfft256_wg_kernel<MODE, TW, NT, W, STG>: workgroup-cooperative radix-256 pass, W = 4 / 8 waves; STG only with MODE 0
#define TFFT_COL_WG256_W(X, W)                                                                               \
  X(0, 0, false, W, false) X(0, 0, false, W, true) X(0, 0, true, W, false) X(0, 0, true, W, true)            \
  X(0, 1, false, W, false) X(0, 1, false, W, true) X(0, 1, true, W, false) X(0, 1, true, W, true)            \
  X(1, 0, false, W, false) X(1, 0, true, W, false) X(1, 1, false, W, false) X(1, 1, true, W, false)          \
  X(1, 2, false, W, false) X(1, 2, true, W, false)
#define TFFT_COL_WG256(X) TFFT_COL_WG256_W(X, 4) TFFT_COL_WG256_W(X, 8)
// colfft512_wg_kernel<MODE, TW, SC, PLAIN> and colfft1024_wg_kernel<MODE, TW, SC, PLAIN>; SC = "scale once" read-out of a final pass
#define TFFT_COL_512(X)                                                                                      \
  X(0, 0, false, false) X(0, 0, false, true) X(0, 1, false, false) X(0, 1, false, true) X(1, 0, false, false) \
  X(1, 0, false, true) X(1, 0, true, false) X(1, 1, false, false) X(1, 1, false, true) X(1, 2, false, false)  \
  X(1, 2, false, true)
#define TFFT_COL_1024(X)                                                                                     \
  X(0, 0, false, false) X(0, 0, false, true) X(0, 1, false, false) X(0, 1, false, true) X(1, 0, false, false) \
  X(1, 0, false, true) X(1, 0, true, false) X(1, 1, false, false) X(1, 1, false, true)
// colfft512r_wg_kernel<W, SC, PF, PLAIN>: two-round radix-512 pass (PF = next tile prefetched through registers: the 8-wave form)
#define TFFT_COL_512R(X)                                                                                     \
  X(8, false, true, false) X(8, false, true, true) X(8, true, true, false) X(4, false, false, false)         \
  X(4, false, false, true) X(4, true, false, false)

// collat256_kernel<MODE, TW, CG, HH, PP>: radix-256 pass for work that does not fill the chip (collat.hpp): 16 CG columns per
// workgroup, a column group's stage 2 split over HH waves and PP = 1 or 2 workgroups
#define TFFT_COL_LAT_S(X, CG, HH, PP) X(0, 0, CG, HH, PP) X(0, 1, CG, HH, PP) X(1, 0, CG, HH, PP) X(1, 1, CG, HH, PP)
#define TFFT_COL_LAT(X)                                                                                      \
  TFFT_COL_LAT_S(X, 4, 2, 1) TFFT_COL_LAT_S(X, 2, 2, 1) TFFT_COL_LAT_S(X, 1, 4, 1) TFFT_COL_LAT_S(X, 2, 2, 2) \
  TFFT_COL_LAT_S(X, 1, 4, 2)

enum : uint32_t { kFamWave = 1, kFamWg256 = 2, kFam512 = 3, kFam512R = 4, kFam1024 = 5, kFamLat = 6 };
using ColKernel = void (*)(colfft::Args);
struct ColRow {
  uint32_t key;
  ColKernel fn;
  uint32_t threads, lds;
  const char* name;
};
constexpr uint32_t col_key(uint32_t fam, int a, int b, int c, int d, int e = 0) {
  return (fam << 20) | (static_cast<uint32_t>(a) << 16) | (static_cast<uint32_t>(b) << 12) | (static_cast<uint32_t>(c) << 8) |
         (static_cast<uint32_t>(d) << 4) | static_cast<uint32_t>(e);
}
const ColRow kColTable[] = {
#define X(MODE, TW, STAGE, LUT)                                                                                      \
  {col_key(kFamWave, MODE, TW, STAGE, LUT), colfft::colfft256_kernel<MODE, TW, STAGE, LUT>, k4096::kThreads, colfft::kLdsBytes, \
   "colfft::colfft256_kernel<" #MODE ", " #TW ", " #STAGE ", " #LUT ">"},
    TFFT_COL_WAVE(X)
#undef X
#define X(MODE, TW, NT, W, STG)                                                                                      \
  {col_key(kFamWg256, MODE, TW, NT, W, STG), colfft::colfft256_wg_kernel<MODE, TW, NT, W, STG>, 64 * W, colfft::WgGeom<W>::kLds,   \
   "colfft::colfft256_wg_kernel<" #MODE ", " #TW ", " #NT ", " #W ", " #STG ">"},
    TFFT_COL_WG256(X)
#undef X
#define X(MODE, TW, SC, PLAIN)                                                                                       \
  {col_key(kFam512, MODE, TW, SC, PLAIN), colfft::colfft512_wg_kernel<MODE, TW, SC, PLAIN>, k4096::kThreads, colfft::kWg512LdsBytes, \
   "colfft::colfft512_wg_kernel<" #MODE ", " #TW ", " #SC ", " #PLAIN ">"},
    TFFT_COL_512(X)
#undef X
#define X(MODE, TW, SC, PLAIN)                                                                                       \
  {col_key(kFam1024, MODE, TW, SC, PLAIN), colfft::colfft1024_wg_kernel<MODE, TW, SC, PLAIN>, k4096::kThreads, colfft::kWg1024LdsBytes, \
   "colfft::colfft1024_wg_kernel<" #MODE ", " #TW ", " #SC ", " #PLAIN ">"},
    TFFT_COL_1024(X)
#undef X
#define X(W, SC, PF, PLAIN)                                                                                          \
  {col_key(kFam512R, W, SC, PF, PLAIN), colfft::colfft512r_wg_kernel<W, SC, PF, PLAIN>, 64 * W, colfft::wg512r_lds_bytes<W>(),  \
   "colfft::colfft512r_wg_kernel<" #W ", " #SC ", " #PF ", " #PLAIN ">"},
    TFFT_COL_512R(X)
#undef X
#define X(MODE, TW, CG, HH, PP)                                                                                      \
  {col_key(kFamLat, MODE, TW, CG, HH, PP), colfft::collat256_kernel<MODE, TW, CG, HH, PP>, colfft::LatGeom<CG, HH, PP>::kThreads, \
   colfft::LatGeom<CG, HH, PP>::kLds, "colfft::collat256_kernel<" #MODE ", " #TW ", " #CG ", " #HH ", " #PP ">"},
    TFFT_COL_LAT(X)
#undef X
};
constexpr size_t kColRows = sizeof(kColTable) / sizeof(kColTable[0]);

inline const ColRow* col_row(uint32_t key) {
  for (const ColRow& r : kColTable)
    if (r.key == key) return &r;
  return nullptr;
}

// the one launch site of every column kernel (lds_bytes = 0: the row's own LDS size)
int launch_col_row(const Launch& L, const tfft_plan* p, uint32_t key, uint32_t grid, const colfft::Args& a, uint32_t lds_bytes = 0) {
  const ColRow* const r = col_row(key);
  if (!r) return fail(TFFT_ERR_ARG, "internal error: column kernel " + std::to_string(key) + " is not in the dispatch table");
  return launch(L, p->device, r->fn, kname(r->name), dim3(grid), dim3(r->threads), lds_bytes ? lds_bytes : r->lds, a);
}

// per-wave kernel: 8 waves per workgroup, one 16-column tile per wave and round
int launch_col_wave(const Launch& L, const tfft_plan* p, int mode, int tw, bool stage, bool lut, const colfft::Args& a) {
  const uint32_t blocks_needed = (a.tasks + k4096::kWavesPerBlock - 1) / k4096::kWavesPerBlock;
  static const uint32_t iters_dflt = env_iters("TFFT_COL_ITERS", 1000000);
  const uint32_t grid = pick_grid(blocks_needed, p->num_cus, plan_iters(p->launch_iters, iters_dflt));
  return launch_col_row(L, p, col_key(kFamWave, mode, tw, stage, tw == colfft::kTwNone ? false : lut), grid, a);
}

// workgroup-cooperative radix-256 kernel, W = 4 or 8 waves
int launch_col_wg(const Launch& L, const tfft_plan* p, int mode, int tw, int w, const colfft::Args& a_in) {
  const uint32_t cols = 16u * static_cast<uint32_t>(w);
  colfft::Args a = a_in;
  uint64_t blocks = (a.tasks / a.groups) * a.pitch / cols;
  if (const SlabCtx* const slab = L.slab) {   // a slab of the pass's columns (whole blocks: the distributed plan checks the divisibility)
    if (slab->col_first % cols || slab->col_count % cols || tw != colfft::kTwFourStep)
      return fail(TFFT_ERR_ARG, "internal error: column slab not a whole number of blocks of a four-step pass");
    a.blk_first = static_cast<uint32_t>(slab->col_first / cols);
    a.blk_count = static_cast<uint32_t>(slab->col_count / cols);
    blocks = a.blk_count;
  }
  // non-temporal copy-in and row stores unless the plan's cache policy says plain (tfft_plan_cache_policy, TFFT_VARIANT_COL_CACHED);
  // columns-on-lanes form: staged full-row stores (TFFT_VARIANT_UNSTAGED_STORES: direct 16-byte pieces)
  const bool nt = !p->plain_acc;
  const bool stg = mode == colfft::kColsOnLanes && !(p->variant & TFFT_VARIANT_UNSTAGED_STORES);
  const uint32_t key = col_key(kFamWg256, mode, tw, nt, w, stg);
  static const uint32_t iters_dflt = env_iters("TFFT_COLWG_ITERS", 1000000);
#ifdef TFFT_DEBUG_KERNELS
  // experiment knob: TFFT_WG4_ONE_PER_CU=1 launches the 4-wave workgroups with so much dynamic LDS (96 KiB) that only ONE fits a CU:
  // the same kernel at one wave per SIMD instead of two (what a radix-1024 pass with 128-column tiles would have to run at).
  // Round 4, against the static partition: +3 ... +10 % on one box; against today's default (8 generations of two per CU), as a
  // variant bit in one process: -3 ... -20 % (profiles/r4_one_wave_per_simd.txt): not a launch shape worth keeping.
  static const bool one_per_cu = env_iters("TFFT_WG4_ONE_PER_CU", 0) != 0;
  if (one_per_cu && w == 4)
    return launch_col_row(L, p, key, gens_grid(blocks, static_cast<uint32_t>(p->num_cus), p->launch_iters, env_iters("TFFT_GENS", 1)), a, 96 * 1024);
#endif
  const uint32_t capacity = static_cast<uint32_t>(p->num_cus * (8 / w));
  const uint32_t grid = iters_dflt != 1000000u ? pick_grid(blocks, static_cast<int>(capacity), plan_iters(p->launch_iters, iters_dflt))
                                               : rounds_grid(blocks, capacity, p->launch_iters);
  return launch_col_row(L, p, key, grid, a);
}

// which (MODE, TW) a radix-256 pass needs: the four-step form, columns on lanes for the first pass of a plain transform
// (Ns = 1), columns in registers otherwise
inline void col_mode_tw(const tfft_plan* p, const Pass& ps, const colfft::Args& a, int& mode, int& tw) {
  if (p->tw4_modulus) {
    mode = colfft::kColsInRegs;
    tw = colfft::kTwFourStep;
    return;
  }
  mode = a.ns_f == 1 ? colfft::kColsOnLanes : colfft::kColsInRegs;
  tw = ps.tw_next ? colfft::kTwNext : colfft::kTwNone;
}

int launch_col(const Launch& L, const tfft_plan* p, const Pass& ps, Planes src, Planes dst) {
  colfft::Args a;
  a.in_re = reinterpret_cast<const uint16_t*>(src.re);
  a.in_im = reinterpret_cast<const uint16_t*>(src.im);
  a.out_re = reinterpret_cast<uint16_t*>(dst.re);
  a.out_im = reinterpret_cast<uint16_t*>(dst.im);
  a.in_stride = src.stride;
  a.out_stride = dst.stride;
  const uint64_t radix = static_cast<uint64_t>(ps.radix);   // 256, or 512 (columns-in-registers form only)
  a.pitch = (p->n / radix) * p->inner;
  a.ns_f = ps.ns * p->inner;
  a.ns_f_shift = static_cast<uint32_t>(ilog2(a.ns_f));
  a.groups = static_cast<uint32_t>(a.pitch / 16);
  a.tasks = static_cast<uint32_t>(a.groups * p->batch);
  a.inner_shift = static_cast<uint32_t>(ilog2(p->inner));
  a.ns = ps.ns;
  a.tw_lo = p->d_tw_lo;
  a.tw_hi = p->d_tw_hi;
  a.tables = static_cast<const uint8_t*>(p->d_tables);
  a.n_mask = (p->tw4_modulus ? p->tw4_modulus : p->n) - 1;
  a.tw_scale = ps.tw_scale;
  a.comb_scale = ps.scale;
  a.tw4_col0 = p->tw4_col0;
  const bool first_pass = &ps == &p->passes[0];
  a.in_seg_shift = first_pass ? p->in_seg_shift : 31;
  a.in_seg_gap = first_pass ? p->in_seg_gap : 0;
  a.blk_first = 0;
  a.blk_count = 0;
  a.out_pitch_shift = static_cast<uint32_t>(ilog2(ps.ns * p->inner));
  a.out_seg_shift = 31;
  a.out_seg_gap = 0;
  a.out_col0 = 0;
  a.out_base = 0;
  if (const SlabCtx* const slab = L.slab) {
    if (!(p->tw4_modulus && ps.radix == 256 && p->passes.size() == 1))
      return fail(TFFT_ERR_ARG, "internal error: a column slab needs a single four-step radix-256 pass");
    a.out_pitch_shift = slab->out_pitch_shift;
    a.out_seg_shift = slab->out_seg_shift;
    a.out_seg_gap = slab->out_seg_gap;
    a.out_col0 = slab->col_first;
    a.out_base = slab->out_base;
  }
#ifdef TFFT_DEBUG_KERNELS
  a.wg_times = nullptr;
  if (debug_variants_enabled())          // measurement hook of tools/exp_wg_end_times.py
    if (const char* e = std::getenv("TFFT_WG_TIMES_PTR"))     // (one block of 16 x 8192 words per pass of the plan)
      a.wg_times = reinterpret_cast<unsigned long long*>(std::strtoull(e, nullptr, 0)) + (&ps - &p->passes[0]) * 16 * 8192;
  a.copy_only = (p->variant & kDbgCopyOnly) ? 1u : 0u;
#endif
  a.out_row_shift = p->out_row_shift;
  a.out_sub_shift = p->out_sub_shift;
  a.out_sub_stride = p->out_sub_stride;
  a.a_shift = 0;
  a.t_mask = 0;
  a.n_over_t = 1;
  a.inv_t = 1.0;
  if (ps.tw_next) {
    // next pass: radix R', Ns'' = ns * 256; it wants w_T^(i' k''), T = Ns'' R', on element
    // o = rest (ns_f 256) + k ns_f + kprev_f:  k'' = k ns + kprev,  i' = o / (n_f / R') = rest >> a_shift
    const uint64_t t = ps.ns * radix * static_cast<uint64_t>(ps.next_radix);
    a.t_mask = t - 1;
    a.n_over_t = p->n / t;
    a.inv_t = 1.0 / static_cast<double>(t);
    a.a_shift = static_cast<uint32_t>(ilog2(p->n / (static_cast<uint64_t>(ps.next_radix) * ps.ns * radix)));
  }
  const bool plain = p->plain_acc;
  const bool sc = ps.scale != 1.0f;              // TFFT_SCALE_ONCE, last pass: the single factor in fp32 at the read-out / combine
  if (radix == 1024 || radix == 512) {
    // (plan creation only emits these passes where the geometry fits: pitch, and ns_f unless it is 1, multiples of 64)
    const uint64_t blocks = (a.tasks / a.groups) * a.pitch / 64;
    const uint32_t grid = gens_grid(blocks, static_cast<uint32_t>(p->num_cus), p->launch_iters, kGensCol8);
    const uint32_t fam = radix == 1024 ? kFam1024 : kFam512;
    if (a.ns_f == 1) return launch_col_row(L, p, col_key(fam, colfft::kColsOnLanes, ps.tw_next ? colfft::kTwNext : colfft::kTwNone, false, plain), grid, a);
    if (radix == 512 && p->tw4_modulus) return launch_col_row(L, p, col_key(fam, colfft::kColsInRegs, colfft::kTwFourStep, false, plain), grid, a);
    if (ps.tw_next) return launch_col_row(L, p, col_key(fam, colfft::kColsInRegs, colfft::kTwNext, false, plain), grid, a);
    if (radix == 512 && (((a.pitch == 256 || a.pitch == 512) && a.ns_f % 128 == 0) != ((p->variant & TFFT_VARIANT_FLIP_RADIX512_KERNEL) != 0))) {
      // last pass of a plan / 2D column pass by the two-round kernel (colfft512r.hpp). A/B in one process on MI355X, 8 GiB per
      // launch (profiles/r3_ab_colfft512r.txt): the 128-column two-round form is 2-4 % faster than the 8-wave single-round
      // kernel at row pitches of 256 and 512 columns (2^18 = 512 x 512: 335 -> 342 Gsamples/s) and at 2048, 2-4 % slower at
      // 128, 1024 and 4096 (the 2D column pass); the default follows that, TFFT_VARIANT_FLIP_RADIX512_KERNEL flips the choice
      // 128-column tiles (256-byte row segments, one 8-wave workgroup per CU) where the geometry allows and TFFT_VARIANT_COL_WG4
      // does not ask for 4-wave workgroups; otherwise 64-column tiles, two 4-wave workgroups per CU
      const bool w8 = !(p->variant & TFFT_VARIANT_COL_WG4) && a.pitch % 128 == 0 && a.ns_f % 128 == 0;
      const uint32_t grid2 = gens_grid(w8 ? blocks / 2 : blocks, static_cast<uint32_t>((w8 ? 1 : 2) * p->num_cus), p->launch_iters, kGensCol8);
      return launch_col_row(L, p, col_key(kFam512R, w8 ? 8 : 4, sc, w8, !sc && plain), grid2, a);
    }
    return launch_col_row(L, p, col_key(fam, colfft::kColsInRegs, colfft::kTwNone, sc, !sc && plain), grid, a);
  }
  int mode, tw;
  col_mode_tw(p, ps, a, mode, tw);
  // default: stores straight from registers (8- / 16-byte pieces); TFFT_VARIANT_COL_WAVE_STAGED: stage the output through
  // LDS (16-byte coalesced stores). Measured in one process on MI355X: direct wins at 2^16 and 2^20, staging at 2^13.
  // workgroup-cooperative form (full 256-byte row segments) whenever the geometry allows; TFFT_VARIANT_COL_PER_WAVE
  // (or either per-wave option) forces the per-wave kernel
  const bool wg_allowed = !(p->variant & kVarColPerWave);
  // per-wave kernel: LDS-staged stores, and twiddles from v_sin / v_cos (TFFT_VARIANT_COL_WAVE_SINCOS) instead of the two-level tables
  const bool stage = p->variant & TFFT_VARIANT_COL_WAVE_STAGED, lut = !(p->variant & TFFT_VARIANT_COL_WAVE_SINCOS);
  const uint64_t entries = a.tasks / a.groups;
  // narrow pitch (N = 256 pitch contiguous, columns-on-lanes form): a workgroup spans 128 / pitch whole batch
  // entries; entries that do not fill a workgroup go to the per-wave kernel in a second launch.
  // (a few entries of 64 columns, the first pass of a small batch of 2^14 = 256 x 64: the latency kernel below)
  const bool lat_narrow = (a.pitch == 64 || a.pitch == 32) && entries <= 64 && tw != colfft::kTwFourStep && !(p->variant & TFFT_VARIANT_NO_LATENCY_KERNEL);
  if (wg_allowed && a.ns_f == 1 && a.pitch >= 16 && a.pitch < 128 && !lat_narrow) {
    const uint64_t per = 128 / a.pitch;
    const uint64_t main_entries = entries - entries % per;
    if (main_entries) {
      colfft::Args am = a;
      am.tasks = static_cast<uint32_t>(main_entries * a.groups);
      const int rc = launch_col_wg(L, p, mode, tw, 8, am);
      if (rc || main_entries == entries) return rc;
      a.in_re += main_entries * a.in_stride;
      a.in_im += main_entries * a.in_stride;
      a.out_re += main_entries * a.out_stride;
      a.out_im += main_entries * a.out_stride;
      a.tasks = static_cast<uint32_t>((entries - main_entries) * a.groups);
    }
    if (a.pitch % 64 == 0) return launch_col_wg(L, p, mode, tw, 4, a);   // 64 columns: one 4-wave workgroup per entry
    return launch_col_wave(L, p, mode, tw, false, true, a);
  }
  const bool wg8_ok = (a.pitch % 128 == 0) && (a.ns_f == 1 || a.ns_f % 128 == 0);
  const bool wg4_ok = (a.pitch % 64 == 0) && (a.ns_f == 1 || a.ns_f % 64 == 0);
  // Work that does not fill the chip (the reference's single-transform benchmark, FFTBenchSinlge.cu): up to 64 blocks of 64
  // columns (2^20 samples per pass) -> the latency kernel (collat.hpp: one memory round trip before the block is in LDS, a column
  // group's stage 2 split over waves on different SIMDs). TFFT_VARIANT_NO_LATENCY_KERNEL keeps the throughput kernels (A/B, tuner).
  // Device time per execution, latency / throughput kernels (profiles/r5_small_scan.txt): 2^16 x 1: 8.8 / 14.3 us, x 16: 13.1 /
  // 16.3; 2^18 x 1 as 256 x 256 x 4: 12.8 / 18.1; 2^20 x 1: 18.4 / 22.2. Beyond 64 blocks the sign depends on the pass (2^16 x 32:
  // 20.0 / 17.7, 2^21 x 1: 26.0 / 28.7, 2^17 x 32: 26.7 / 23.3): the throughput kernels keep everything from there on. 128 blocks
  // still win by 7-9 % wherever a row is at least 512 columns wide (2^21 x 1, 2^20 x 2: 26.5 / 28.6, 2^19 x 4: 26.1 / 28.0, 2^18 x 8
  // as 256 x 256 x 4: 25.9 / 27.6) and lose 13 % at a pitch of 256 (2^16 x 32, above).
  // (in units of 16 columns: a pitch of 32, the first pass of 2^13 = 256 x 32, is two 16-column blocks per entry)
  const uint64_t blocks16 = entries * a.pitch / 16, blocks64 = (blocks16 + 3) / 4;
  const bool lat_geom = wg4_ok || (a.pitch == 32 && a.ns_f == 1);
  // (tfft_plan_opts.launch_iters shapes the grids of the grid-stride kernels; this kernel's grid is one workgroup per block either way,
  // so a launch shape never changes WHICH kernel runs, and with it the bits: test_launch_shape_never_changes_results)
  if (wg_allowed && lat_geom && tw != colfft::kTwFourStep && !(p->variant & TFFT_VARIANT_NO_LATENCY_KERNEL) && blocks64 <= (a.pitch >= 512 ? 128u : 64u)) {
    // Workgroup shape (column groups of 16 per workgroup, waves per column group): stage 2 is bound by instruction issue, so the
    // finer the split the shorter the pass - until the row segments get too narrow for the memory system (32-byte segments over
    // 4 MiB: loads land after 2.3 us instead of 0.9, tools/lat_probe). One box, device time per transform, shapes 4 x 2 / 2 x 2 /
    // 1 x 4 (profiles/r5_lat_shapes.txt): 2^16: 12.4 / 9.5 / 8.6 us, 2^18: 16.3 / 13.1 / 12.5, 2^19: 17.2 / 14.5 / 14.8, 2^20:
    // 20.0 / 18.2 / 21.7.
    const int cgs = blocks64 <= 16 ? 1 : 2;
    const int hh = cgs == 1 ? 4 : 2;
    // ... and beyond the workgroup: PP = 2 workgroups per block, each with the whole block in its LDS and half of the stage-2 tiles
    // and of the rows to store, while that still leaves one workgroup per CU (one wave per SIMD is the point) and every wave keeps
    // two tiles. One box, PP = 1 / 2 / 4 (profiles/r5_lat_shapes.txt, second part): 2^16 8.54 / 8.24 us, 2^17 11.50 / 11.18, 2^18
    // 12.45 / 12.25, 2^19 14.39 / 13.80 / 14.17, 2^20 18.12 / 17.77 / 20.23, 2^21 (256 workgroups already) 26.0 / 27.5: 2-4 %, and
    // four-way loses what two-way gains (every partner repeats the loads and stage 1). The partners READ the same block and WRITE
    // disjoint bytes of dst: never for a pass in place.
    const uint32_t wgs = static_cast<uint32_t>(blocks16 / cgs);
    const int pp = (a.in_re != a.out_re && a.in_im != a.out_im && wgs * 2 <= static_cast<uint32_t>(p->num_cus) && 16 / (hh * 2) >= 2) ? 2 : 1;
    int cgs_used = cgs, hh_used = hh, pp_used = pp;
#ifdef TFFT_DEBUG_KERNELS
    if (const uint32_t shape = env_iters("TFFT_LAT_SHAPE", 0)) {      // experiment knob, digits CG HH [PP]: 42, 22, 14; 222, 142
      const uint32_t two = shape >= 100 ? shape / 10 : shape;
      cgs_used = static_cast<int>(two / 10);
      hh_used = static_cast<int>(two % 10);
      pp_used = shape >= 100 ? static_cast<int>(shape % 10) : 1;
    }
#endif
    return launch_col_row(L, p, col_key(kFamLat, mode, tw, cgs_used, hh_used, pp_used),
                          static_cast<uint32_t>(blocks16 / cgs_used) * static_cast<uint32_t>(pp_used), a);
  }
  // TFFT_VARIANT_COL_WG4: 4-wave workgroups (two per CU) instead of one 8-wave workgroup
  static const uint32_t wg4_max_pitch_lanes = env_iters("TFFT_WG4_MAX_PITCH", 1024);          // experiment knobs
  // (the columns-in-registers form, whose output is staged behind two more barriers, gains from two workgroups per
  // CU up to a pitch of 16384: 2^20 x 1024 221.6 -> 228.9 Gsamples/s, 2^22 215.5 -> 220.1; beyond that the 128-byte
  // segments lose more than the overlap gives: 2^24 194.6 -> 170.8)
  static const uint32_t wg4_max_pitch_regs = env_iters("TFFT_WG4_MAX_PITCH_INREGS", 16384);
  // Round 3, today's kernels (rotated work distribution, conflict-free staging), W = 4 against W = 8 on one box
  // (profiles/r3_ab_w4_w8.txt): the plain and next-pass-twiddle forms prefer 8-wave workgroups (256-byte segments) from a pitch
  // of 512 columns on: +4 % at 512 (last pass of 2^17: 345 -> 358 Gsamples/s), +6 % at 1024, +10 % at 4096, +4 % at 16384; at 256
  // the two 4-wave workgroups per CU still win by 2-3 %. The four-step form is within 1 % either way and keeps its threshold.
  const uint32_t wg4_regs = p->tw4_modulus ? wg4_max_pitch_regs : std::min<uint32_t>(wg4_max_pitch_regs, 256u);
  const uint32_t wg4_max_pitch = (a.ns_f == 1) ? wg4_max_pitch_lanes : wg4_regs;
  // ... also when 8-wave workgroups would leave CUs idle (single long transforms: 2^20 x 1 is 32 blocks of 128 columns)
  const bool few_blocks = entries * a.pitch / 128 < static_cast<uint64_t>(p->num_cus);
  if (wg_allowed && wg4_ok && ((p->variant & TFFT_VARIANT_COL_WG4) || !wg8_ok || a.pitch <= wg4_max_pitch || few_blocks))
    return launch_col_wg(L, p, mode, tw, 4, a);
  if (wg_allowed && wg8_ok) return launch_col_wg(L, p, mode, tw, 8, a);
  return launch_col_wave(L, p, mode, tw, stage, lut, a);
}

template <int R>
int launch_pass(const Launch& L, int device, const stockham::PassArgs& a, uint64_t batch) {
  const uint64_t grid = (a.m_f * batch + stockham::kBlock - 1) / stockham::kBlock;
  return launch(L, device, stockham::pass_kernel<R>, kname("stockham::pass_kernel", R), dim3(static_cast<uint32_t>(grid)), dim3(stockham::kBlock), 0, a);
}

template <int R>
int launch_pass_pair(const Launch& L, int device, const stockham::PassArgs& a, uint64_t batch) {
  const uint64_t grid = ((a.m_f / 2) * batch + stockham::kBlock - 1) / stockham::kBlock;
  return launch(L, device, stockham::pass_pair_kernel<R>, kname("stockham::pass_pair_kernel", R), dim3(static_cast<uint32_t>(grid)), dim3(stockham::kBlock), 0, a);
}

int launch_stockham_pass(const Launch& L, const tfft_plan* p, const Pass& ps, Planes src, Planes dst) {
  stockham::PassArgs a;
  a.in_re = src.re;
  a.in_im = src.im;
  a.out_re = dst.re;
  a.out_im = dst.im;
  a.in_stride = src.stride;
  a.out_stride = dst.stride;
  a.n = p->n;
  const int R = ps.radix;
  a.m_f = (p->n / R) * p->inner;
  a.ns = ps.ns * p->inner;
  a.inner_shift = static_cast<uint32_t>(ilog2(p->inner));
  a.skip_tw = ps.skip_tw ? 1u : 0u;
  a.tw_mul = p->n / (ps.ns * R);
  a.batch = p->batch;
  a.m_shift = static_cast<uint32_t>(ilog2(a.m_f));
  a.tw_lo = p->d_tw_lo;
  a.tw_hi = p->d_tw_hi;
  a.scale = ps.scale;
  // pre-twiddled radix-2/4/8 pass with an even sub-transform length: two butterflies per thread, 4-byte accesses
  // (measured +5 % on the whole 2^17 transform; for radix 16 it is neutral in 1D and -6 % on the 2D column pass, so
  // those keep one butterfly per thread). TFFT_VARIANT_PACKED keeps the one-butterfly kernel.
  if (a.skip_tw && a.ns >= 2 && a.m_f >= 2 && R <= 8 && !(p->variant & TFFT_VARIANT_PACKED)) {
    switch (R) {
      case 2: return launch_pass_pair<2>(L, p->device, a, p->batch);
      case 4: return launch_pass_pair<4>(L, p->device, a, p->batch);
      default: return launch_pass_pair<8>(L, p->device, a, p->batch);
    }
  }
  // Workgroup-cooperative final pass (stockham::tail_coop_kernel): radix 128 always (plan_passes emits it only as 2^15 = 256 x 128),
  // radix 64 / 32 for the last pass of 2^14 = 256 x 64 / 2^13 = 256 x 32 while the batch is small (16-byte row segments: a large batch keeps the
  // butterfly-per-thread kernel, whose accesses are whole lines)
  const bool coop_geom = a.skip_tw && a.ns == a.m_f && a.m_f % stockham::kCoopCols == 0 && p->inner == 1;
  if (R == 128 || ((R == 64 || R == 32) && coop_geom && p->n == 256ull * R && p->batch <= 16 && !(p->variant & TFFT_VARIANT_PACKED))) {
    if (!coop_geom) return fail(TFFT_ERR_ARG, "internal error: radix-128 pass outside its geometry");
    const dim3 grid(static_cast<uint32_t>(a.m_f / stockham::kCoopCols * p->batch));
    if (R == 128) return launch(L, p->device, stockham::tail_coop_kernel<128>, kname("stockham::tail_coop_kernel", 128), grid, dim3(256), 0, a);
    if (R == 64) return launch(L, p->device, stockham::tail_coop_kernel<64>, kname("stockham::tail_coop_kernel", 64), grid, dim3(128), 0, a);
    return launch(L, p->device, stockham::tail_coop_kernel<32>, kname("stockham::tail_coop_kernel", 32), grid, dim3(64), 0, a);
  }
  switch (R) {
    case 2: return launch_pass<2>(L, p->device, a, p->batch);
    case 4: return launch_pass<4>(L, p->device, a, p->batch);
    case 8: return launch_pass<8>(L, p->device, a, p->batch);
    case 32: return launch_pass<32>(L, p->device, a, p->batch);
    case 64: return launch_pass<64>(L, p->device, a, p->batch);
    default: return launch_pass<16>(L, p->device, a, p->batch);
  }
}

// Blocks of tfft_plan_workspace_bytes() in a workspace the LIBRARY allocates: two for a chain with an odd number >= 3 of passes
// (in place it runs IN -> A -> B -> ... -> IN, launch_chain), one for every other plan. The count follows from the plan alone, so
// an owned workspace is allocated once, by tfft_plan_prepare or the first execution of any kind, and never grows, moves or is
// freed by a later execution: tfft_exec stays launches only, capturable, and a captured graph keeps a valid pointer.
inline size_t owned_workspace_blocks(const tfft_plan* p) {
  const size_t np = p->passes.size();
  return (np >= 3 && (np % 2) == 1) ? 2 : 1;
}

// The plan's workspace and how many blocks it holds, read under ws_mutex; allocates the library's own if there is none yet. A
// walk (`dry`) allocates nothing: the address is a placeholder and the block count is what an execution would find. `needed`:
// the calling execution uses the workspace; one that does not (it only settles it for the executions after it) takes a caller's
// workspace that is too small as zero blocks and leaves the error to the execution that needs them.
int acquire_workspace(const tfft_plan* p, bool needed, bool dry, _Float16** w, size_t* blocks) {
  std::lock_guard<std::mutex> lock(p->ws_mutex);
  const size_t block = tfft_plan_workspace_bytes(p);
  *w = dry ? kFakeWorkspace : static_cast<_Float16*>(p->ws);
  *blocks = 0;
  if (block == 0) return TFFT_OK;
  if (p->ws) {
    // (an owned workspace has owned_workspace_blocks() blocks from the start, so only a caller's can be too small)
    if (p->ws_bytes < block) return needed ? fail(TFFT_ERR_WORKSPACE, "workspace handed to tfft_plan_set_workspace is too small") : TFFT_OK;
    *blocks = p->ws_bytes / block;
    return TFFT_OK;
  }
  *blocks = owned_workspace_blocks(p);
  if (dry) return TFFT_OK;
  TFFT_HIP(hipMalloc(&p->ws, block * *blocks));
  p->ws_bytes = block * *blocks;
  p->ws_owned = true;
  *w = static_cast<_Float16*>(p->ws);
  return TFFT_OK;
}

int launch_chain(const Launch& L, const tfft_plan* p, const void* in_re, const void* in_im, void* out_re, void* out_im) {
  const bool dry = L.mode != Mode::Run;
  if (p->sub_col) {
    // TFFT_ORDER_TRANSPOSED: column pass in -> planar workspace, row pass workspace -> out (in place is fine: the input
    // has been read completely before the row pass writes)
    _Float16* w = nullptr;
    size_t ws_blocks = 0;
    const int wrc = acquire_workspace(p, true, dry, &w, &ws_blocks);
    if (wrc) return wrc;
    _Float16* const w_im = w + p->chunk * p->n;
    const _Float16 *i_re = static_cast<const _Float16*>(in_re), *i_im = static_cast<const _Float16*>(in_im);
    _Float16 *o_re = static_cast<_Float16*>(out_re), *o_im = static_cast<_Float16*>(out_im);
    for (uint64_t b0 = 0; b0 < p->batch; b0 += p->chunk) {
      const bool tail = p->batch - b0 < p->chunk;
      const tfft_plan* const col = tail ? p->sub_col_tail : p->sub_col;
      const tfft_plan* const row = tail ? p->sub_row_tail : p->sub_row;
      const uint64_t io = b0 * p->in_stride, oo = b0 * p->out_stride;
      int rc;
      if (p->rows_first) {
        // transposed-order INPUT: N1 contiguous N2-point transforms per [N1][N2] block (output twiddle w_N^(k1 q) in their
        // epilogue) into the workspace, then one radix-N1 column pass over k1 writes X[q + N2 p] in natural order
        rc = launch_chain(L, row, i_re + io, i_im + io, w, w_im);
        if (rc) return rc;
        rc = launch_chain(L, col, w, w_im, o_re + oo, o_im + oo);
      } else {
        rc = launch_chain(L, col, i_re + io, i_im + io, w, w_im);
        if (rc) return rc;
        rc = launch_chain(L, row, w, w_im, o_re + oo, o_im + oo);
      }
      if (rc) return rc;
      if (L.mode == Mode::OptIn && !p->sub_col_tail) break;      // (LDS opt-in: one walk per distinct sub-plan is enough)
    }
    return TFFT_OK;
  }
  int np = static_cast<int>(p->passes.size());
  if (kDebugBuild && (p->variant & kDbgPasses)) np = std::min(np, (p->variant & kDbgPasses) >> kDbgPassesShift);   // debugging aid: run only the first passes
  if (single_kernel(p)) {
    const PassKind kind = p->passes[0].kind;
    const int rc = kind == PassKind::K4096
                       ? launch_k4096(L, p, in_re, in_im, out_re, out_im, p->in_map, p->out_map)
                   : kind == PassKind::K4096R
                       ? launch_k4096r(L, p, p->passes[0].radix, in_re, in_im, out_re, out_im, p->in_map, p->out_map)
                       : (kind == PassKind::K256
                              ? launch_k256(L, p, in_re, in_im, out_re, out_im, p->in_map, p->out_map)
                              : launch_k256r(L, p, p->passes[0].radix, in_re, in_im, out_re, out_im, p->in_map, p->out_map));
    if (rc) return rc;
    if (!dry) TFFT_HIP(hipGetLastError());
    return TFFT_OK;
  }
  const uint64_t nf = p->n * p->inner;
  Planes IN{const_cast<_Float16*>(static_cast<const _Float16*>(in_re)),
            const_cast<_Float16*>(static_cast<const _Float16*>(in_im)), p->in_stride};
  Planes OUT{static_cast<_Float16*>(out_re), static_cast<_Float16*>(out_im), p->out_stride};
  const bool in_place = (in_re == out_re) || (in_im == out_im);
  // Targets alternate OUT / SCR so that the last pass writes OUT. SCR is the input
  // block when the reference's "input is scratch" contract allows it and the chain
  // does not start by overwriting what it reads; otherwise the plan's workspace.
  const bool odd = (np % 2) == 1;
  const bool use_in_as_scratch = !p->preserve_input && !in_place && odd;
  Planes SCR = IN;
  Planes SRC = IN;
  // In place with an odd number (>= 3) of passes: the chain needs a third buffer, IN -> A -> B -> ... -> OUT (= IN): the second
  // block of the workspace. The library's own workspace of such a plan has two blocks from its allocation on
  // (owned_workspace_blocks), and so has a caller's of twice tfft_plan_workspace_bytes. With a caller's single block, and for a
  // single pass, the chain starts from a copy of the input instead (one more launch: the reference's own single-transform
  // benchmark runs 2^18 and 2^21 in place, results_in_results_ = false, and paid 3 / 11 us for that copy).
  // The workspace is settled by the first execution of any kind, also by one that does not use it (input as scratch, a single
  // pass out of place): an in-place execution after it finds its blocks and allocates nothing (tfft.h, tfft_plan_prepare).
  Planes SCR_B{};
  bool two_blocks = false;
  const bool needs_ws = !use_in_as_scratch && (np > 1 || in_place);
  // (a walk: a workspace address of its own, so that every pass sees the pointer relations of an execution)
  _Float16* w = nullptr;
  size_t ws_blocks = 0;
  if (needs_ws || !p->out_of_place_only) {
    const int rc = acquire_workspace(p, needs_ws, dry, &w, &ws_blocks);
    if (rc) return rc;
  }
  if (needs_ws) {
    two_blocks = in_place && odd && np >= 3 && ws_blocks >= 2;
    SCR = Planes{w, w + nf, 2 * nf};
    if (two_blocks) {
      _Float16* w2 = w + p->batch * 2 * nf;
      SCR_B = Planes{w2, w2 + nf, 2 * nf};
    } else if (in_place && odd) {
      // chain IN -> OUT would read and write the same block: start from a copy of the [RE | IM] blocks. tfft_exec_inverse hands
      // the planes in exchanged, IM in front of RE: the same blocks, copied from the lower pointer, and the chain reads the copy
      // with the planes in the caller's order.
      const _Float16* const re = static_cast<const _Float16*>(in_re);
      const _Float16* const im = static_cast<const _Float16*>(in_im);
      const bool swapped = im + nf == re;
      if (p->in_stride != 2 * nf || !(im == re + nf || swapped))
        return fail(TFFT_ERR_ARG, "in-place execution of this length with a workspace of one block needs the [RE | IM] block layout "
                                  "(planes N apart, batch stride 2N)");
      const uint64_t n32 = p->batch * nf;          // 4 bytes per complex sample
      const int rc = launch(L, p->device, stockham::copy_kernel, kname("stockham::copy_kernel"), dim3(static_cast<uint32_t>(std::min<uint64_t>((n32 + 255) / 256, 8192))),
                            dim3(stockham::kBlock), 0, reinterpret_cast<const uint32_t*>(swapped ? im : re), reinterpret_cast<uint32_t*>(w), n32);
      if (rc) return rc;
      SRC = swapped ? Planes{w + nf, w, 2 * nf} : SCR;
    }
  }
  Planes cur = SRC;
  for (int i = 0; i < np; ++i) {
    const bool to_out = ((np - 1 - i) % 2) == 0;
    const Planes dst = two_blocks ? (i + 1 == np ? OUT : ((i % 2) ? SCR_B : SCR)) : (to_out ? OUT : SCR);
    const Pass& ps = p->passes[i];
    if (ps.kind == PassKind::Col256) {
      const int rc = launch_col(L, p, ps, cur, dst);
      if (rc) return rc;
    } else {
      const int rc = launch_stockham_pass(L, p, ps, cur, dst);
      if (rc) return rc;
    }
    cur = dst;
  }
  if (!dry) TFFT_HIP(hipGetLastError());
  return TFFT_OK;
}

// bytes between the stand-in planes of a walk over p
inline uint64_t walk_span(const tfft_plan* p) { return 4 * (p->batch * std::max(p->in_stride, p->out_stride) + p->n * p->inner); }

// The OptIn walk: runs the launch logic of a plan without launching, so that every kernel it can select gets its LDS opt-in now,
// a failure surfaces from tfft_plan_create and tfft_exec makes no runtime call besides the launches.
int prepare_kernels(const tfft_plan* p) {
  const WalkPtrs f = walk_ptrs(walk_span(p));
  return launch_chain(Launch::opt_in(), p, f.in_re, f.in_im, f.out_re, f.out_im);
}

// The Record walk: walk(L) runs a piece of launch logic over a recording context and appends the kernels an execution of it
// launches to `names`, in launch order.
template <class Walk>
int record_walk(std::vector<std::string>& names, Walk&& walk) {
  Recorder rec{&names, {}};
  const int rc = walk(Launch::record(rec));
  if (rc == TFFT_OK && !rec.mismatch.empty()) return fail(TFFT_ERR_ARG, "internal error: kernel name " + rec.mismatch);
  return rc;
}

// The kernels one execution of p launches (tfft_plan_kernels): out of place over the data pointers of prepare_kernels, or in place
// over the [RE | IM] block layout.
int record_kernels(const tfft_plan* p, bool in_place, std::vector<std::string>& names) {
  if (in_place && p->in_stride != p->out_stride) return fail(TFFT_ERR_ARG, "in-place execution needs equal input and output batch strides");
  const WalkPtrs f = in_place ? walk_ptrs_in_place(2 * p->n * p->inner) : walk_ptrs(walk_span(p));
  return record_walk(names, [&](const Launch& L) { return launch_chain(L, p, f.in_re, f.in_im, f.out_re, f.out_im); });
}

// names -> buf, one per line; returns how many
int put_kernel_lines(const std::vector<std::string>& names, char* buf, size_t bytes) {
  std::string out;
  for (const std::string& k : names) out += k + "\n";
  if (!buf || out.size() + 1 > bytes) return fail(TFFT_ERR_ARG, "buffer too small (" + std::to_string(out.size() + 1) + " bytes needed)");
  std::memcpy(buf, out.c_str(), out.size() + 1);
  return static_cast<int>(names.size());
}
