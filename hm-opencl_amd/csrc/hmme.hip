// hmme.hip -- host side of the C ABI declared in include/hmme.h (see that header for the
// reference interface each entry point replaces).  Plain HIP runtime; no OpenCL, no fallback path.
#include "../../include/hmme.h"
#include "../../include/hmme_test.h"

#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <type_traits>
#include <vector>

#include "me_kernels.hpp"

using hmme::MeJob;
using hmme::MeJob16;
using hmme::RefSet;

namespace {
constexpr int kMarginX = 128;  // samples; >= 72 needed by clipMv's bounds (+3 for dword staging); keeps CTU rows 64B-aligned
constexpr int kMarginY = 80;   // TComPicYuv: maxCUHeight + 16 (reference TComPicYuv.cpp:91-92)
constexpr int kWinPitch = 1024;  // per-CTU path: bytes per packed window row (>= 2 * (257 + 63) + 8)
constexpr int kRefineHalo = 4;   // samples the 8-tap interpolation reaches beyond the window on every side (TComInterpolationFilter.cpp:170-260)
constexpr int kWinRows = 2 * 128 + 1 + 63 + 2 * kRefineHalo;
// per-CTU call block: up to 64 MeJob16, the job's first strip (always 0), the 593-entry 64-bit merge table (all ones),
// the 64 x 64 current block (1 or 2 bytes per sample), the caller's integer MVs (refine-only call), the packed window.
// kCallFracJob: the whole-window MeJob of the refinement kernel (jobs[] may hold window tiles)
constexpr size_t kCallJobs = 0, kCallFirst = 1536, kCallFracJob = 1600, kCallBest = 2048, kCallCtu = 7168, kCallImv = 15360, kCallWin = 17920;
constexpr int kCallMaxJobs = 64;
static_assert(sizeof(MeJob16) * kCallMaxJobs <= kCallFirst && kCallFracJob + sizeof(MeJob) <= kCallBest && kCallBest + 8 * HMME_NUM_CTU_PARTS <= kCallCtu &&
              kCallCtu + 64 * 64 * 2 <= kCallImv && kCallImv + 4 * HMME_NUM_CTU_PARTS <= kCallWin && kCallWin % 256 == 0, "per-CTU call block layout");
// pinned result block: 593 MVs, 593 SADs, completion word of the search; 593 quarter-pel MVs, 593 costs, completion word of the refinement
constexpr size_t kResMv = 0, kResSad = 4 * HMME_NUM_CTU_PARTS, kResDone = 8 * HMME_NUM_CTU_PARTS, kResQmv = kResDone + 64,
                 kResCost = kResQmv + 4 * HMME_NUM_CTU_PARTS, kResDone2 = kResCost + 4 * HMME_NUM_CTU_PARTS, kResBytes = kResDone2 + 64;
// per workgroup of the 16-bit path -> 2 workgroups per CU
constexpr size_t kLdsBudget16 = 78 * 1024;
// LDS window pitch of the 16-bit kernel in dwords -- a template parameter of the kernel (the odd row of a row pair is addressed by
// an immediate).  A lane reads dwords 3 * (lane in row) + 0..33 of its window row, lanes-per-row L = ceil(ceil(wx / 2) / 3), so a
// row needs 3 * (L - 1) + 34 dwords; the pitch also decides which banks the rows of one wave-wide read share (64 lanes cover 1.5 .. 6
// window rows): with pitch == 3 * L (mod 32) the 64 lanes form ONE stride-3 progression over the 32 banks and a ds_read2_b32 costs
// its minimum.  Measured (profiles/archive/r02Y_pdw_sweep.txt, GSAD/s at 2160p 10-bit): SR 128 -- 160: 1 782, 161: 1 812, 162: 1 780,
// 164..170: 1 698..1 724; SR 64 -- 130: 1 687, 97..106 otherwise: 1 630..1 651.  Four pitches are compiled, the right ones for the
// full windows of SR 32 / 64 / 96 / 128 (round 2 had two, and SR 32 / 96 ran 5 % below the tuned ranges); any other window takes the
// smallest pitch that holds it, preferring the right residue (pick_pdw16).
constexpr int kPdw16[4] = {65, 130, 131, 161};
constexpr int kPdw16Large = kPdw16[3];
inline int pdw16_index(int pdw) { return pdw == kPdw16[0] ? 0 : pdw == kPdw16[1] ? 1 : pdw == kPdw16[2] ? 2 : 3; }
// pitch for windows up to wx candidates wide
int pick_pdw16(int wx) {
  const int lanes = (((wx + 1) >> 1) + 2) / 3, need = 3 * (lanes - 1) + 34, want = (3 * lanes) & 31;
  int best = kPdw16Large;
  bool best_match = false;
  for (int i = 3; i >= 0; --i) {
    if (kPdw16[i] < need) continue;
    const bool match = (kPdw16[i] & 31) == want;
    if (match || !best_match) { best = kPdw16[i]; best_match = match; }   // descending: the smallest fitting one wins among equals
  }
  return best;
}
thread_local std::string g_create_error;   // hmme_last_error(NULL): per host thread, like the contexts themselves
constexpr size_t lds_bytes16_c(int pdw, int strip_rows) { return (size_t)(2 * 594 + 4 + (strip_rows + 63) * pdw) * 4; }
static_assert(lds_bytes16_c(kPdw16Large, 1) <= kLdsBudget16, "a one-row strip fits the LDS budget (strips_for terminates)");
}  // namespace

// One growable device allocation: every device buffer a context or a plane owns.  The capacity is in bytes; a use site takes a typed
// view (as<T>).  grow: free and allocate anew -- hipFree synchronises the whole device
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  template <typename T> T* as() const { return (T*)p; }
  hipError_t grow(size_t bytes) {
    if (p) hipFree(p);
    p = nullptr; cap = 0;
    const hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess) cap = bytes;
    return e;
  }
};
// the device buffers of a context: hmme_ctx::buf, freed by one loop in hmme_destroy
enum Buf {
  kCall,        // per-CTU path: the call block (kCall* offsets above), allocated by hmme_create
  kFlag,        // int[4]: [0] synchronous uploads, [1] asynchronous uploads, [2] take_flag's result; hmme_create
  kJobs,        // frame path scratch: MeJob[] or MeJob16[] of the searches (jobs_tag)
  kFirstStrip,  // int[]: the jobs' first strips
  kFracJobs,    // MeJob[] of the refinement launches that read a table (+ the job counter of the job-walking mode; frac_jobs_tag)
  kBest,        // [jobs][593] 64-bit merge table of the split / strip / segment launches (best_clean)
  kWp0, kWp1, kWp2, kWp3,   // weighted whole-picture calls: u16 copies of the planes of one launch (below)
  kWwin,        // per-CTU calls with weighted prediction: the weighted copy of the staged window (the search's); first use
  kFracCover,   // uint16[]: fractional refinement, the slots covering each 8x8 / 4x4 position, same for every CTU; first use
  kWpEst,       // hmme_plane_stats / hmme_wp_estimate / hmme_wp_estimate_420: the 64-bit sums of one call (kWpSet* below); first use
  kStage,       // the staging arena of the synchronous, host-array forms (Stage)
  kNumBufs
};

struct hmme_ctx {
  int device = 0;
  int sr_max = 64;
  uint32_t lambda_q16 = 0;
  std::string err;
  bool print_errors = true;   // hmme_set_error_printing
  std::string info;
  hipStream_t stream = nullptr;   // private stream of the synchronous entry points
  // frame-path scratch (job tables, merge table, cover table) is shared by every call of the context: a call on another stream
  // than the previous one first waits (stream-side) for that one's last use
  // ONE event is recorded behind the kernels of a launch (ring of kLaunchEvents, launch_end): it marks the scratch's last use and the last
  // read of every plane the launch took (hmme_plane::read_done points into the ring).  A ring entry that has been recorded again
  // since stands for a LATER point of the same chain of launches -- every launch of a context is ordered behind the one before it
  // through the scratch -- so a waiter on a recycled entry waits longer than it had to, never too little.
  static constexpr int kLaunchEvents = 64;
  hipEvent_t launch_ev[kLaunchEvents] = {};
  unsigned launch_seq = 0;
  hipEvent_t scratch_done = nullptr;   // the ring entry of the last launch
  hipStream_t scratch_stream = nullptr;
  bool scratch_used = false;
  // per-CTU path: one device block and its pinned host mirror -- jobs, first-strip index, merge table preset, current
  // block, window -- so that a call is one upload, the kernels, one download (layout: kCall* offsets below)
  DevBuf buf[kNumBufs];
  uint8_t* h_call = nullptr;
  uint8_t* h_call_dev = nullptr;  // device-side address of h_call (mapped pinned memory)
  uint8_t* h_res = nullptr;       // 593 MVs (int16 x, y), 593 SADs, then the completion word: pinned host memory the finalize kernel writes
  uint8_t* d_res = nullptr;       // ... and its device-side address
  uint32_t call_seq = 0;
  // A job table is a function of the picture size, the search range, the CTU range, the number of pairs and the predictors.  Launches
  // WITHOUT predictors (d_pred_q == null: the zero predictor of the reference's own call) of the same geometry on the same stream find
  // the table of the launch before still in place and skip the kernels that write it -- one kernel launch less per search step.
  // `buf` / `buf2`: the allocations the table lives in (a reallocation invalidates it)
  struct TableTag {
    bool valid = false;
    int w = 0, h = 0, bit_depth = 0, sr = 0, first = 0, count = 0, pairs = 0;
    const void* buf = nullptr; const void* buf2 = nullptr; void* stream = nullptr;
    bool same(const TableTag& o) const {
      return valid && o.valid && w == o.w && h == o.h && bit_depth == o.bit_depth && sr == o.sr && first == o.first && count == o.count && pairs == o.pairs &&
             buf == o.buf && buf2 == o.buf2 && stream == o.stream;
    }
  };
  TableTag jobs_tag;              // what kJobs / kFirstStrip hold (searches)
  TableTag frac_jobs_tag;         // ... and kFracJobs
  int wg_slots = 512;     // search workgroups resident at once: 2 per CU (VGPRs of the search kernels, LDS of the 16-bit one)
  bool best_clean = false;   // every entry of kBest is all ones: me_finalize16_kernel resets what it decodes, so only a table that is new, has
                             // grown or was left behind by a failed launch needs the preset (merge_table)
  bool lds_optin[8] = {false, false, false, false, false, false, false, false};
  int num_cus = 0;
  bool frac_lds_optin[6] = {false, false, false, false, false, false};   // per build of me_frac_kernel (FracBuild::index)
  int frac_wg_per_cu[6] = {0, 0, 0, 0, 0, 0};   // same index: workgroups of that me_frac_kernel a CU holds (runtime occupancy query, first use)
  // kWp0..kWp3, weighted whole-picture calls (hmme_search_pairs_w_device / hmme_refine_pairs_w_device): one copy per pair, grown on
  // demand -- kWp0 weighted reference planes and kWp1 biased CTU-blocked current pictures (search); kWp2 raw reference planes widened
  // from 8 bit and kWp3 biased padded current pictures (refinement).  Scratch like the job tables: scratch_acquire / launch_end
  uint8_t* wp(int i) const { return buf[kWp0 + i].as<uint8_t>(); }
  uint8_t* d_call() const { return buf[kCall].as<uint8_t>(); }
};

struct hmme_plane {
  hmme_ctx* ctx = nullptr;
  int width = 0, height = 0;
  int bit_depth = 8;
  int bps = 1;            // bytes per sample: 1 (8-bit path) or 2 (9..12 bit)
  int pitch = 0;          // bytes per row, multiple of 256
  int rows = 0;           // height + 2 * kMarginY
  uint8_t* d_data = nullptr;
  // the picture area once more, CTU by CTU: block (cx, cy) = 64 rows x 64 samples, contiguous, raster order of CTUs, partial edge CTUs
  // completed by edge replication -- what the search kernels read the CURRENT picture from (scalar loads at immediate offsets, whatever
  // the picture's size: me_kernels.hpp me_prefetch_cur).  Written by every fill right behind the padded plane (plane_fill).
  uint8_t* d_blocks = nullptr;
  int ctus_x = 0, n_ctu = 0;
  DevBuf stage;   // device staging for uploads
  hipEvent_t filled = nullptr;      // recorded after the last fill; readers on another stream wait for it
  hipStream_t fill_stream = nullptr;
  bool fill_pending = false;
  // the event of the last launch that reads the plane (an entry of the context's ring, hmme_ctx::launch_ev: not owned); a refill on
  // another stream waits for it (write after read).  mutable: reading a plane does not change what it holds
  mutable hipEvent_t read_done = nullptr;
  mutable hipStream_t read_stream = nullptr;
  mutable bool read_pending = false;
  // hmme_plane_stats: sum of the picture's samples and of |sample - normDC| of the contents last filled in; every fill drops them
  mutable bool stats_valid = false;
  mutable int64_t stats_dc = 0, stats_ac = 0;
  const uint8_t* origin() const { return d_data + (size_t)kMarginY * pitch + (size_t)kMarginX * bps; }
};

namespace {

int fail(hmme_ctx* ctx, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (ctx) ctx->err = buf; else g_create_error = buf;
  if (!ctx || ctx->print_errors) fprintf(stderr, "hmme: ERROR: %s\n", buf);   // TEncOpenCL::checkError prints too (TEncOpenCL.h:93-101)
  return code;
}

#define HIP_TRY(ctx, call)                                                                              \
  do {                                                                                                  \
    hipError_t e_ = (call);                                                                             \
    if (e_ != hipSuccess) return fail(ctx, HMME_ERR_DEVICE, "%s -> %s", #call, hipGetErrorString(e_));   \
  } while (0)

// `b` holds at least `bytes`.  *moved: the allocation was replaced (or lost, where this fails) -- what it held is gone
int ensure(hmme_ctx* ctx, DevBuf& b, size_t bytes, size_t grow_to = 0, bool* moved = nullptr) {
  if (moved) *moved = false;
  if (bytes <= b.cap) return HMME_OK;
  // hipFree synchronises the whole device -- in the middle of a streaming pipeline that stalls the copy and download streams.  A
  // scratch that has to grow therefore grows to `grow_to` at once (the callers pass what kMaxRefs pairs of this picture size need:
  // KBs to a few MB), so a steady stream meets this path on its first launch of a picture size and never again.
  if (grow_to > bytes) bytes = grow_to;
  if (moved) *moved = true;
  HIP_TRY(ctx, b.grow(bytes));
  return HMME_OK;
}

// ---- the staging arena of the synchronous, host-array forms -----------------------------------------------------------
// Every hmme_*_frame* entry point has the same shape: lay its host arrays out in one device buffer (kStage), grow it, copy up, run the
// *_device form on ctx->stream, copy down, wait.  A call describes its arrays as items (in / out / image), begin() places and uploads
// them, at() hands the device addresses to the launch, end() downloads and makes the call's one hipStreamSynchronize.  The arena grows to
// exactly what a call needs and never shrinks; an error returns without a wait.
constexpr size_t kStageAlign = 256;   // every item starts like an allocation of its own would (the select kernels need 8 bytes)
// the pure layout: item i of bytes[i] at offsets[i], a multiple of kStageAlign; an empty item takes no room.  Returns the arena's size
size_t stage_layout(const size_t* bytes, int n, size_t* offsets) {
  size_t total = 0;
  for (int i = 0; i < n; ++i) {
    offsets[i] = total;
    total += (bytes[i] + kStageAlign - 1) & ~(kStageAlign - 1);
  }
  return total;
}
struct Stage {
  struct Item {
    size_t bytes = 0;                       // on the device; 0: the caller has no such array, at() is null
    const void* up = nullptr;               // linear in: the host array
    void* down = nullptr;                   // linear out and image: the host array
    size_t parts = 0, part_bytes = 0, off = 0, len = 0;   // linear out: of each of `parts` equal parts the bytes [off, off + len) come back
    size_t row = 0, rows = 0, stride = 0;   // image: rows of `row` bytes, `stride` bytes apart at the host, `pitch` (packed: `row`) on the device
    size_t pitch = 0;
    const void* up_image = nullptr;         // image that only goes up (the caller's is const): `down` is null
  };
  hmme_ctx* ctx;
  std::vector<Item> items;
  std::vector<size_t> at_;
  explicit Stage(hmme_ctx* c) : ctx(c) {}
  int add(const Item& it) { items.push_back(it); return (int)items.size() - 1; }
  // each returns the item's index for at().  A null host pointer reserves nothing
  int in(const void* host, size_t bytes) {
    Item it;
    if (host && bytes) { it.bytes = bytes; it.up = host; }
    return add(it);
  }
  int out(void* host, size_t part_bytes, size_t off, size_t len, size_t parts = 1) {
    Item it;
    if (host && len) { it.bytes = parts * part_bytes; it.down = host; it.parts = parts; it.part_bytes = part_bytes; it.off = off; it.len = len; }
    return add(it);
  }
  // in and out: uploaded before the launch, so samples the kernel does not write come back as they were
  int image(void* host, size_t row, size_t rows, size_t stride, size_t pitch = 0) {
    Item it;
    if (host && row * rows) { it.pitch = pitch ? pitch : row; it.bytes = it.pitch * rows; it.down = host; it.row = row; it.rows = rows; it.stride = stride; }
    return add(it);
  }
  // in only: an image the launch reads
  int image_in(const void* host, size_t row, size_t rows, size_t stride) {
    Item it;
    if (host && row * rows) { it.pitch = row; it.bytes = row * rows; it.up_image = host; it.row = row; it.rows = rows; it.stride = stride; }
    return add(it);
  }
  uint8_t* at(int i) const { return items[i].bytes ? ctx->buf[kStage].as<uint8_t>() + at_[i] : nullptr; }
  int begin() {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<size_t> bytes;
    for (const Item& it : items) bytes.push_back(it.bytes);
    at_.resize(items.size());
    const int rc = ensure(ctx, ctx->buf[kStage], stage_layout(bytes.data(), (int)bytes.size(), at_.data()));
    if (rc) return rc;
    for (size_t i = 0; i < items.size(); ++i) {
      const Item& it = items[i];
      if (it.row) HIP_TRY(ctx, hipMemcpy2DAsync(at((int)i), it.pitch, it.down ? it.down : it.up_image, it.stride, it.row, it.rows, hipMemcpyHostToDevice, ctx->stream));
      if (it.up) HIP_TRY(ctx, hipMemcpyAsync(at((int)i), it.up, it.bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    return HMME_OK;
  }
  int end() {
    for (size_t i = 0; i < items.size(); ++i) {
      const Item& it = items[i];
      if (it.row && it.down) HIP_TRY(ctx, hipMemcpy2DAsync(it.down, it.stride, at((int)i), it.pitch, it.row, it.rows, hipMemcpyDeviceToHost, ctx->stream));
      for (size_t p = 0; p < it.parts; ++p) {
        const size_t o = p * it.part_bytes + it.off;
        HIP_TRY(ctx, hipMemcpyAsync((uint8_t*)it.down + o, at((int)i) + o, it.len, hipMemcpyDeviceToHost, ctx->stream));
      }
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return HMME_OK;
  }
};

// cross-stream ordering (see hmme.h "Streams"): scratch of the context, contents of a plane
int scratch_acquire(hmme_ctx* ctx, hipStream_t s) {
  if (ctx->scratch_used && ctx->scratch_stream != s) HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->scratch_done, 0));
  return HMME_OK;
}
int launch_end(hmme_ctx* ctx, hipStream_t s) {
  hipEvent_t ev = ctx->launch_ev[ctx->launch_seq++ % hmme_ctx::kLaunchEvents];
  HIP_TRY(ctx, hipEventRecord(ev, s));
  ctx->scratch_done = ev; ctx->scratch_stream = s; ctx->scratch_used = true;
  return HMME_OK;
}
int plane_wait(hmme_ctx* ctx, const hmme_plane* pl, hipStream_t s) {
  if (pl->fill_pending && pl->fill_stream != s) HIP_TRY(ctx, hipStreamWaitEvent(s, pl->filled, 0));
  return HMME_OK;
}
// a search / refinement on `s` has been enqueued that reads `pl`.  One event holds the LAST read only, so a read on a new stream
// first makes that stream wait for the previous reader (plane_read_chain, before the launch's event is recorded): the event then
// covers both.  plane_read_mark: the launch's event (launch_end) is the plane's last read
int plane_read_chain(hmme_ctx* ctx, const hmme_plane* pl, hipStream_t s) {
  if (pl->read_pending && pl->read_stream != s) HIP_TRY(ctx, hipStreamWaitEvent(s, pl->read_done, 0));
  return HMME_OK;
}
void plane_read_mark(hmme_ctx* ctx, const hmme_plane* pl, hipStream_t s) {
  pl->read_done = ctx->scratch_done; pl->read_stream = s; pl->read_pending = true;
}
// before `s` overwrites the plane (or its staging buffer): the last fill and the last reader, if they ran on other streams
int plane_write_wait(hmme_ctx* ctx, const hmme_plane* pl, hipStream_t s) {
  if (pl->fill_pending && pl->fill_stream != s) HIP_TRY(ctx, hipStreamWaitEvent(s, pl->filled, 0));
#ifndef HMME_TEST_NO_WAR_WAIT   // tools/build_variant.sh nowar -DHMME_TEST_NO_WAR_WAIT: shows that the two-stream refill test fails without this wait
  if (pl->read_pending && pl->read_stream != s) HIP_TRY(ctx, hipStreamWaitEvent(s, pl->read_done, 0));
#endif
  return HMME_OK;
}

// the A/B knobs of the environment (include/hmme.h, "Environment"), read once per process
struct Knobs { int tail_parts = 0, tail_launches = 0, frac_grid = 0; bool frac_job_table = false, trace = false; };
const Knobs& knobs() {
  static const Knobs k = [] {
    const auto num = [](const char* name) { const char* v = std::getenv(name); return v ? std::atoi(v) : 0; };
    return Knobs{num("HMME_TAIL_PARTS"), num("HMME_TAIL_LAUNCHES"), num("HMME_FRAC_GRID"), std::getenv("HMME_FRAC_JOB_TABLE") != nullptr, std::getenv("HMME_TRACE") != nullptr};
  }();
  return k;
}

// ---- 8-bit path --------------------------------------------------------------------------------------
RefSet one_ref(const uint8_t* base) {
  RefSet r;
  for (int i = 0; i < hmme::kMaxRefs; ++i) r.base[i] = base;
  return r;
}

// Progress-based wave priorities of the search kernels (me_search_kernel, me_search16_kernel): the kernel whose workgroups are whole CTU
// searches always runs with them (+8 % on a single-round 1080p launch, +2 % at 2160p: the lonely ends of each CU's last workgroups);
// the launches of many small workgroups -- split tasks, window tiles, 16-bit strips -- only while the launch is a few rounds of the
// chip's workgroup slots (720p +5 %, 1080p 10-bit +5 %; config 5's 16 rounds of strips lost 0.8 % with them:
// profiles/r05d_fair_priority_ab.txt).
int fair_prio(const hmme_ctx* ctx, int workgroups, bool whole_jobs) {
  return (whole_jobs || workgroups <= 4 * ctx->wg_slots) ? 1 : 0;
}

// The one way a search launch picks its cost function: f is called with std::integral_constant<int, FEN> and names its kernel with it.
template <class F>
auto with_fen(int fen, F&& f) {
  return fen ? f(std::integral_constant<int, 1>{}) : f(std::integral_constant<int, 0>{});
}

// me_search_kernel<FEN, SPLIT, PK> over n_wg workgroups.  SPLIT = 0: whole jobs (MeJob), results straight into d_mv / d_sad; 1 and 2 (below) merge into `best`.
// PK (me_pk_body): with FEN 1 the kernel that holds the packed-minimum twin and its marker-free body wherever the context's lambda passes me_pk2_gate
// (lambda <= 224: HM's lambdas over QP 22..37 lie far inside), the twin alone up to me_pk_gate and with FEN 0, the 32-bit tree beyond
template <int SPLIT>
int launch_search8(hmme_ctx* ctx, const RefSet& cur, int cur_ctus_x, const RefSet& ref, int ref_pitch, const void* d_jobs, int n_wg, int fen,
                   int16_t* d_mv, uint32_t* d_sad, unsigned long long* best, int n_seg_jobs, hipStream_t stream) {
  if (n_wg <= 0) return HMME_OK;
  return with_fen(fen, [&](auto f) -> int {
    constexpr int FEN = decltype(f)::value;
    const int body = hmme::me_pk_body(ctx->lambda_q16, FEN);
    auto kernel = body ? hmme::me_search_kernel<FEN, SPLIT, 1> : hmme::me_search_kernel<FEN, SPLIT, 0>;
    if constexpr (FEN == 1) {
      if (body == 2) kernel = hmme::me_search_kernel<1, SPLIT, 2>;
    }
    hipLaunchKernelGGL(kernel, dim3(n_wg), dim3(hmme::kThreads), 0, stream, cur, cur_ctus_x, ref,
                       ref_pitch, d_jobs, ctx->lambda_q16, d_mv, d_sad, best, fair_prio(ctx, n_wg, SPLIT == 0), n_seg_jobs);
    HIP_TRY(ctx, hipGetLastError());
    return HMME_OK;
  });
}

int finalize_best(hmme_ctx* ctx, unsigned long long* d_best, const MeJob16* d_jobs, const int* d_first_strip, int n_jobs, int16_t* d_mv,
                  uint32_t* d_sad, hipStream_t stream);

// the 64-bit merge table of a split / strip / tile launch: the caller's (already all ones), or the context's (kBest) grown and preset here
int merge_table(hmme_ctx* ctx, int n_jobs, unsigned long long* preset, hipStream_t stream, unsigned long long** table) {
  if (preset) { *table = preset; return HMME_OK; }
  DevBuf& best = ctx->buf[kBest];
  bool moved;
  const int rc = ensure(ctx, best, sizeof(unsigned long long) * HMME_NUM_CTU_PARTS * (size_t)n_jobs,
                        n_jobs > 64 ? sizeof(unsigned long long) * HMME_NUM_CTU_PARTS * (size_t)n_jobs * 2 : 0, &moved);
  if (moved) ctx->best_clean = false;
  if (rc) return rc;
  if (!ctx->best_clean) HIP_TRY(ctx, hipMemsetAsync(best.p, 0xFF, best.cap, stream));
  ctx->best_clean = false;   // until the launch's finalize_best has been enqueued (it sets every entry it decodes back to all ones)
  *table = best.as<unsigned long long>();
  return HMME_OK;
}

// 8-bit split mode: n_jobs * n_split workgroups, each runs a slice of its CTU's tasks and merges through the merge table
int launch_search8_split(hmme_ctx* ctx, const RefSet& cur, int cur_ctus_x, const RefSet& ref, int ref_pitch, const MeJob16* d_jobs,
                         const int* d_first_strip, int n_jobs, int n_split, int fen, int16_t* d_mv, uint32_t* d_sad,
                         hipStream_t stream, unsigned long long* preset_best = nullptr, bool finalize = true) {
  if (n_jobs <= 0) return HMME_OK;
  unsigned long long* best = nullptr;
  int rc = merge_table(ctx, n_jobs, preset_best, stream, &best);
  if (rc) return rc;
  rc = launch_search8<1>(ctx, cur, cur_ctus_x, ref, ref_pitch, d_jobs, n_jobs * n_split, fen, nullptr, nullptr, best, 0, stream);
  if (rc) return rc;
  return finalize ? finalize_best(ctx, best, d_jobs, d_first_strip, n_jobs, d_mv, d_sad, stream) : HMME_OK;
}

// 8-bit segment mode: the tasks of n_jobs jobs in n_wg equal segments (table: me_seg_table_*), merged through `best` (preset by the caller)
int launch_search8_segments(hmme_ctx* ctx, const RefSet& cur, int cur_ctus_x, const RefSet& ref, int ref_pitch, const void* d_table,
                            const int* d_first_strip, int n_jobs, int n_wg, int fen, int16_t* d_mv, uint32_t* d_sad, hipStream_t stream,
                            unsigned long long* best) {
  if (n_jobs <= 0 || n_wg <= 0) return HMME_OK;
  const int rc = launch_search8<2>(ctx, cur, cur_ctus_x, ref, ref_pitch, d_table, n_wg, fen, nullptr, nullptr, best, n_jobs, stream);
  if (rc) return rc;
  return finalize_best(ctx, best, hmme::me_seg_table_jobs(d_table, n_wg), d_first_strip, n_jobs, d_mv, d_sad, stream);
}

// ---- 16-bit path -------------------------------------------------------------------------------------

size_t lds_bytes16(int pdw, int strip_rows) { return lds_bytes16_c(pdw, strip_rows); }

// most candidate rows of one strip whose window rows (+ 63) fit the LDS budget
int rows_max16(int pdw) {
  int r = 1;
  while (lds_bytes16(pdw, r + 1) <= kLdsBudget16) ++r;
  return r;
}

// strips of candidate rows so that one strip's window rows fit the LDS budget
constexpr int strips_for(int pdw, int wy_max) {
  int n = 1;
  while (n < wy_max && lds_bytes16_c(pdw, (wy_max + n - 1) / n) > kLdsBudget16) ++n;   // bounded: one-row strips always fit
  return n;
}
// 53 candidate rows fit at the largest pitch, so the tallest window takes 5 strips: the per-CTU deal (ctu_deal) never asks for more workgroups than its job table holds
static_assert(strips_for(kPdw16Large, 2 * HMME_MAX_SEARCH_RANGE + 1) <= kCallMaxJobs, "the strips the LDS needs fit the per-CTU job table");

// f is called with std::integral_constant<int, PDW> of the compiled pitch `pdw` (pick_pdw16)
template <class F>
auto with_pdw16(int pdw, F&& f) {
  switch (pdw16_index(pdw)) {
    case 0: return f(std::integral_constant<int, kPdw16[0]>{});
    case 1: return f(std::integral_constant<int, kPdw16[1]>{});
    case 2: return f(std::integral_constant<int, kPdw16[2]>{});
    default: return f(std::integral_constant<int, kPdw16[3]>{});
  }
}

template <int FEN, int PDW>
int launch16_t(hmme_ctx* ctx, const RefSet& cur, int cur_ctus_x, const RefSet& ref, int ref_pitch, const MeJob16* d_jobs, int n_wg,
               size_t lds, int sh, unsigned long long* d_best, hipStream_t stream) {
  bool& attr_set = ctx->lds_optin[FEN * 4 + pdw16_index(PDW)];   // > 64 KiB of dynamic LDS: opt in once per
  if (!attr_set) {                                                            // kernel and device (= per context)
    HIP_TRY(ctx, hipFuncSetAttribute((const void*)hmme::me_search16_kernel<FEN, PDW>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr_set = true;
  }
  hipLaunchKernelGGL((hmme::me_search16_kernel<FEN, PDW>), dim3(n_wg), dim3(hmme::kThreads16), lds, stream, cur, cur_ctus_x, ref,
                     ref_pitch, d_jobs, ctx->lambda_q16, sh, d_best, fair_prio(ctx, n_wg, false));
  HIP_TRY(ctx, hipGetLastError());
  return HMME_OK;
}

// d_jobs: n_jobs * n_strips MeJob16; results merged in the merge table then decoded into d_mv / d_sad
int launch_search16(hmme_ctx* ctx, const RefSet& cur, int cur_ctus_x, const RefSet& ref, int ref_pitch, const MeJob16* d_jobs,
                    const int* d_first_strip, int n_jobs, int n_wg, int pdw, int strip_rows_max, int fen, int bit_depth,
                    int16_t* d_mv, uint32_t* d_sad, hipStream_t stream, unsigned long long* preset_best = nullptr, bool finalize = true) {
  if (n_jobs <= 0) return HMME_OK;
  unsigned long long* best = nullptr;
  int rc = merge_table(ctx, n_jobs, preset_best, stream, &best);
  if (rc) return rc;
  const size_t lds = lds_bytes16(pdw, strip_rows_max);
  const int sh = bit_depth - 8;
  rc = with_fen(fen, [&](auto f) {
    return with_pdw16(pdw, [&](auto p) { return launch16_t<decltype(f)::value, decltype(p)::value>(ctx, cur, cur_ctus_x, ref, ref_pitch, d_jobs, n_wg, lds, sh, best, stream); });
  });
  if (rc) return rc;
  return finalize ? finalize_best(ctx, best, d_jobs, d_first_strip, n_jobs, d_mv, d_sad, stream) : HMME_OK;
}

int finalize_best(hmme_ctx* ctx, unsigned long long* d_best, const MeJob16* d_jobs, const int* d_first_strip, int n_jobs, int16_t* d_mv,
                  uint32_t* d_sad, hipStream_t stream) {
  const long total = (long)n_jobs * HMME_NUM_CTU_PARTS;
  hipLaunchKernelGGL(hmme::me_finalize16_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, d_best, d_jobs,
                     d_first_strip, n_jobs, ctx->lambda_q16, d_mv, d_sad);
  HIP_TRY(ctx, hipGetLastError());
  if (d_best == ctx->buf[kBest].p) ctx->best_clean = true;   // the launches of a context are one chain (scratch_acquire): the next one finds the table reset
  return HMME_OK;
}

// the CTUs a call handles: ctu_count < 0 = from ctu_first to the end of the picture
int ctu_range(hmme_ctx* ctx, const hmme_frame_params* fp, int n_ctu, int* first, int* count) {
  *first = fp->ctu_first;
  *count = fp->ctu_count < 0 ? n_ctu - fp->ctu_first : fp->ctu_count;
  if (*first < 0 || *count < 0 || *first + *count > n_ctu) return fail(ctx, HMME_ERR_ARG, "CTU range [%d, +%d) outside 0..%d", *first, *count, n_ctu);
  return HMME_OK;
}

int check_frame_args(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* ref, const hmme_frame_params* fp, int* first,
                     int* count) {
  if (!ctx) return HMME_ERR_ARG;
  if (!cur || !ref || !fp) return fail(ctx, HMME_ERR_ARG, "null plane / params");
  // a launch ties the planes it reads to an event of THIS context's ring (plane_read_mark): a plane of another context would be left
  // pointing into that ring after the context is gone
  if (cur->ctx != ctx || ref->ctx != ctx) return fail(ctx, HMME_ERR_ARG, "plane belongs to another context (planes are used with the context that created them)");
  if (cur->width != ref->width || cur->height != ref->height) return fail(ctx, HMME_ERR_ARG, "cur/ref size mismatch");
  if (fp->bit_depth < 8 || fp->bit_depth > 12) return fail(ctx, HMME_ERR_UNSUPPORTED, "bit depth %d outside 8..12", fp->bit_depth);
  if (cur->bit_depth != fp->bit_depth || ref->bit_depth != fp->bit_depth)
    return fail(ctx, HMME_ERR_ARG, "planes hold %d/%d-bit samples, search asks for %d", cur->bit_depth, ref->bit_depth, fp->bit_depth);
  if (fp->search_range < 1 || fp->search_range > ctx->sr_max)
    return fail(ctx, HMME_ERR_ARG, "search range %d outside [1, %d]", fp->search_range, ctx->sr_max);
  return ctu_range(ctx, fp, hmme_num_ctus(cur->width, cur->height), first, count);
}

// Range violations are latched on the device: flag 0 by the synchronous uploads (taken right behind the fill, on its stream), flag 1
// by the asynchronous ones (taken by hmme_upload_status) -- a bad sample of an asynchronous upload can no longer fail the next
// synchronous upload of another, valid plane.  Read and clear are one atomic exchange on the stream (me_take_flag_kernel).
int take_flag(hmme_ctx* ctx, int which, hipStream_t s, int* out) {
  hipLaunchKernelGGL(hmme::me_take_flag_kernel, dim3(1), dim3(1), 0, s, ctx->buf[kFlag].as<int>() + which, ctx->buf[kFlag].as<int>() + 2);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(out, ctx->buf[kFlag].as<int>() + 2, sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  return HMME_OK;
}

template <typename SrcT, typename DstT>
int plane_fill(hmme_plane* pl, const SrcT* d_src, int src_pitch_elems, hipStream_t s, bool check) {
  hmme_ctx* ctx = pl->ctx;
  pl->stats_valid = false;   // hmme_plane_stats: the cached sums describe the previous contents
  int wrc = plane_write_wait(ctx, pl, s);   // the previous fill and the last reader, if on other streams
  if (wrc) return wrc;
  dim3 grid((pl->pitch / 4 + 255) / 256, pl->rows);
  hipLaunchKernelGGL((hmme::me_fill_plane_kernel<SrcT, DstT>), grid, dim3(256), 0, s, pl->d_data, pl->pitch, kMarginX, kMarginY,
                     pl->width, pl->height, d_src, src_pitch_elems, (1 << pl->bit_depth) - 1, ctx->buf[kFlag].as<int>() + (check ? 0 : 1));
  HIP_TRY(ctx, hipGetLastError());
  // ... and the CTU-blocked copy the searches read the current picture from (one more pass over the staged picture: 8 MB at 2160p)
  const long blk_threads = (long)pl->n_ctu * (hmme::kBlkBytes8 * pl->bps / 4);
  hipLaunchKernelGGL((hmme::me_fill_blocks_kernel<SrcT, DstT>), dim3((unsigned)((blk_threads + 255) / 256)), dim3(256), 0, s, pl->d_blocks, pl->ctus_x,
                     pl->n_ctu, pl->width, pl->height, d_src, src_pitch_elems);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(pl->filled, s));
  pl->fill_stream = s; pl->fill_pending = true;
  if (check) {
    int flag = 0;
    const int rc = take_flag(ctx, 0, s, &flag);
    if (rc) return rc;
    if (flag) return fail(ctx, HMME_ERR_RANGE, "plane upload: sample outside [0,%d] for a %d-bit plane", (1 << pl->bit_depth) - 1, pl->bit_depth);
  }
  return HMME_OK;
}

// s == nullptr: the synchronous upload (private stream, range check, returns when the plane is filled); otherwise asynchronous on
// `s` -- the copy runs at PCIe rate only from page-locked memory (hmme_host_register) and a range violation is latched for
// hmme_upload_status
template <typename T>
int plane_upload(hmme_plane* pl, const T* origin, int stride, hipStream_t s, bool sync) {
  if (!pl) return HMME_ERR_ARG;
  hmme_ctx* ctx = pl->ctx;
  if (!origin || stride < pl->width) return fail(ctx, HMME_ERR_ARG, "plane upload: bad origin/stride");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (sync) s = ctx->stream;
  const size_t bytes = sizeof(T) * (size_t)pl->width * pl->height;
  if (pl->stage.cap < bytes && pl->fill_pending) HIP_TRY(ctx, hipEventSynchronize(pl->filled));   // a fill may still be reading the old staging buffer
  int rc = ensure(ctx, pl->stage, bytes);
  if (rc) return rc;
  rc = plane_write_wait(ctx, pl, s);   // the staging buffer is read by the previous fill
  if (rc) return rc;
  HIP_TRY(ctx, hipMemcpy2DAsync(pl->stage.p, sizeof(T) * pl->width, origin, sizeof(T) * (size_t)stride, sizeof(T) * pl->width,
                                pl->height, hipMemcpyHostToDevice, s));
  if (pl->bps == 1) return plane_fill<T, uint8_t>(pl, pl->stage.as<const T>(), pl->width, s, sync);
  return plane_fill<T, uint16_t>(pl, pl->stage.as<const T>(), pl->width, s, sync);
}

}  // namespace

extern "C" {

int hmme_num_ctus(int width, int height) { return ((width + 63) / 64) * ((height + 63) / 64); }

int hmme_create(int device, int sr_max, unsigned flags, hmme_ctx** out) {
  (void)flags;
  if (!out) return fail(nullptr, HMME_ERR_ARG, "hmme_create: out == NULL");
  *out = nullptr;
  if (sr_max < 1 || sr_max > HMME_MAX_SEARCH_RANGE)
    return fail(nullptr, HMME_ERR_UNSUPPORTED, "hmme_create: sr_max %d outside [1, %d]", sr_max, HMME_MAX_SEARCH_RANGE);
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0)
    return fail(nullptr, HMME_ERR_DEVICE, "hmme_create: no HIP device (this engine has no CPU fallback)");
  if (device < 0 || device >= n_dev) return fail(nullptr, HMME_ERR_ARG, "hmme_create: device %d of %d", device, n_dev);
  hipDeviceProp_t prop;
  if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&prop, device) != hipSuccess)
    return fail(nullptr, HMME_ERR_DEVICE, "hmme_create: cannot open device %d", device);
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(nullptr, HMME_ERR_DEVICE, "hmme_create: device %d is %s; the kernels are built for gfx950 only", device, prop.gcnArchName);
  hmme_ctx* ctx = new hmme_ctx;
  ctx->device = device;
  ctx->sr_max = sr_max;
  char info[256];
  // (the marketing name comes from libdrm's amdgpu.ids table, which a minimal install may lack: the string then starts with what the
  // runtime always knows -- the architecture)
  snprintf(info, sizeof info, "%s (%s), %d CUs, %.0f GiB", prop.name[0] ? prop.name : "AMD GPU (no marketing name on this host)", prop.gcnArchName,
           prop.multiProcessorCount, (double)prop.totalGlobalMem / (1 << 30));
  ctx->info = info;
  ctx->wg_slots = 2 * prop.multiProcessorCount;
  ctx->num_cus = prop.multiProcessorCount;
  const size_t win_bytes = (size_t)kWinRows * kWinPitch + 64;
#define CREATE_TRY(call)                                                                                           \
  do {                                                                                                             \
    hipError_t e_ = (call);                                                                                        \
    if (e_ != hipSuccess) { int rc = fail(nullptr, HMME_ERR_NOMEM, "hmme_create: %s -> %s", #call, hipGetErrorString(e_)); hmme_destroy(ctx); return rc; } \
  } while (0)
  CREATE_TRY(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
  for (int i = 0; i < hmme_ctx::kLaunchEvents; ++i) CREATE_TRY(hipEventCreateWithFlags(&ctx->launch_ev[i], hipEventDisableTiming));
  CREATE_TRY(ctx->buf[kCall].grow(kCallWin + win_bytes));
  CREATE_TRY(hipHostMalloc(&ctx->h_call, kCallWin + win_bytes, hipHostMallocMapped));
  CREATE_TRY(hipHostGetDevicePointer((void**)&ctx->h_call_dev, ctx->h_call, 0));
  std::memset(ctx->h_call, 0, kCallWin);
  std::memset(ctx->h_call + kCallBest, 0xFF, 8 * HMME_NUM_CTU_PARTS);
  CREATE_TRY(hipHostMalloc(&ctx->h_res, kResBytes, hipHostMallocMapped));
  std::memset(ctx->h_res, 0, kResBytes);
  CREATE_TRY(hipHostGetDevicePointer((void**)&ctx->d_res, ctx->h_res, 0));
  CREATE_TRY(ctx->buf[kFlag].grow(4 * sizeof(int)));
  CREATE_TRY(hipMemset(ctx->buf[kFlag].p, 0, 4 * sizeof(int)));
#undef CREATE_TRY
  *out = ctx;
  return HMME_OK;
}

void hmme_destroy(hmme_ctx* ctx) {
  if (!ctx) return;
  hipSetDevice(ctx->device);
  if (ctx->stream) { hipStreamSynchronize(ctx->stream); hipStreamDestroy(ctx->stream); }
  for (int i = 0; i < hmme_ctx::kLaunchEvents; ++i)
    if (ctx->launch_ev[i]) hipEventDestroy(ctx->launch_ev[i]);
  for (DevBuf& b : ctx->buf) hipFree(b.p);
  if (ctx->h_call) hipHostFree(ctx->h_call);
  if (ctx->h_res) hipHostFree(ctx->h_res);
  delete ctx;
}

const char* hmme_last_error(const hmme_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }
int hmme_set_error_printing(hmme_ctx* ctx, int on) {
  if (!ctx) return 1;
  const int was = ctx->print_errors ? 1 : 0;
  ctx->print_errors = on != 0;
  return was;
}
const char* hmme_device_info(const hmme_ctx* ctx) { return ctx ? ctx->info.c_str() : ""; }
int hmme_device_index(const hmme_ctx* ctx) { return ctx ? ctx->device : -1; }

int hmme_set_lambda(hmme_ctx* ctx, double lambda) {
  if (!ctx) return HMME_ERR_ARG;
  if (!(lambda >= 0.0)) return fail(ctx, HMME_ERR_ARG, "lambda %g", lambda);
  const double q = std::floor(65536.0 * std::sqrt(lambda));   // TEncOpenCL.h:121 == TComRdCost.cpp:209
  if (!(q < 4294967296.0)) return fail(ctx, HMME_ERR_ARG, "lambda %g: 65536 * sqrt(lambda) does not fit 32 bits", lambda);
  ctx->lambda_q16 = (uint32_t)q;
  return HMME_OK;
}
int hmme_set_lambda_q16(hmme_ctx* ctx, uint32_t q) {
  if (!ctx) return HMME_ERR_ARG;
  ctx->lambda_q16 = q;
  return HMME_OK;
}
uint32_t hmme_get_lambda_q16(const hmme_ctx* ctx) { return ctx ? ctx->lambda_q16 : 0; }

void hmme_params_ocl_compat(hmme_search_params* p, int lt_x, int lt_y, int sr) {
  // TEncOpenCL.cpp:312-313 scans [0, 2*SR] from LT and never reads RB; cl/sad.cl:374-398 prices the MV
  // against (0,0); no row sub-sampling, no bit-depth shift
  p->lt_x = lt_x; p->lt_y = lt_y; p->rb_x = lt_x + 2 * sr; p->rb_y = lt_y + 2 * sr;
  p->pred_x = 0; p->pred_y = 0; p->fen = 0; p->bit_depth = 8; p->shift_free = 1;
}

void hmme_set_search_range(int pred_x_q, int pred_y_q, int sr, int cu_x, int cu_y, int pic_w, int pic_h, int* lt_x,
                           int* lt_y, int* rb_x, int* rb_y) {
  hmme::set_search_range(pred_x_q, pred_y_q, sr, cu_x, cu_y, pic_w, pic_h, *lt_x, *lt_y, *rb_x, *rb_y);
}

// ---- slot layout: closed form of the 593-case switch of TComDataCU::getIndexBlock ------------------------
namespace {
const int kBase2NxN[4] = {588, 560, 448, 0}, kBaseNx2N[4] = {590, 568, 480, 128};      // indexed by depth (CU 64,32,16,8)
const int kBaseAMP[4] = {576, 512, 256, -1}, kBase2Nx2N[4] = {592, 584, 544, 384};

int slot_of(int part_size, int depth, int part_idx, int cx, int cy) {
  const int n = 1 << depth, r = cy * n + cx;
  if (part_idx < 0 || part_idx > 1) return -1;
  switch (part_size) {
    case 0: return part_idx == 0 ? kBase2Nx2N[depth] + r : -1;
    case 1: return kBase2NxN[depth] + cy * 2 * n + part_idx * n + cx;
    case 2: return kBaseNx2N[depth] + cy * 2 * n + 2 * cx + part_idx;
    default: break;
  }
  if (depth == 3) return -1;
  static const int k_of[4][2] = {{0, 3}, {2, 1}, {4, 7}, {6, 5}};   // 2NxnU, 2NxnD, nLx2N, nRx2N x part_idx -> AMP family
  if (part_size < 4 || part_size > 7) return -1;
  return kBaseAMP[depth] + k_of[part_size - 4][part_idx] * n * n + r;
}
}  // namespace

int hmme_slot_index(int part_size, int depth, int part_idx, int abs_z_idx) {
  if (depth < 0 || depth > 3 || abs_z_idx < 0 || abs_z_idx > 255) return -1;
  int bx = 0, by = 0;   // z-order -> raster in 4x4 units
  for (int b = 0; b < 4; ++b) { bx |= ((abs_z_idx >> (2 * b)) & 1) << b; by |= ((abs_z_idx >> (2 * b + 1)) & 1) << b; }
  const int s4 = 16 >> depth;   // CU size in 4x4 units
  if (bx % s4 || by % s4) return -1;
  return slot_of(part_size, depth, part_idx, bx / s4, by / s4);
}

// ---- the table layout of an encoder built with AMP_ENC_SPEEDUP (TypeDef.h:206, :260-261: NUM_CTU_PARTS 425; cl/sad.cl:4-138 `calcSAD`,
// TComDataCU.cpp:3393-4675).  Dead in the reference tree as shipped (the macro is 0), kept as a VIEW of the 593 tables: the same
// rectangles without the AMP shapes.  Bases per CU size 8 / 16 / 32 / 64: 2NxN 0 / 320 / 400 / 420, Nx2N 128 / 352 / 408 / 422,
// 2Nx2N 256 / 384 / 416 / 424; inside a family the order of the 593 layout -- except that the reference's table numbers the two
// parts of the 64x64 2NxN and Nx2N CUs in reverse (part 1 before part 0: TComDataCU.cpp:3396-3410), which is reproduced.
int hmme_slot_index_amp_off(int part_size, int depth, int part_idx, int abs_z_idx) {
  if (part_size < 0 || part_size > 2 || part_idx < 0 || part_idx > 1 || (part_size == 0 && part_idx)) return -1;
  const int full = hmme_slot_index(part_size, depth, part_idx, abs_z_idx);
  if (full < 0) return -1;
  static const int base593[3][4] = {{592, 584, 544, 384}, {588, 560, 448, 0}, {590, 568, 480, 128}};     // [part size][depth]
  static const int base425[3][4] = {{424, 416, 384, 256}, {420, 400, 320, 0}, {422, 408, 352, 128}};
  int in_family = full - base593[part_size][depth];
  if (depth == 0 && part_size != 0) in_family ^= 1;
  return base425[part_size][depth] + in_family;
}

int hmme_amp_off_slot(int index_amp_off) {   // which of the 593 slots holds table entry `index_amp_off` of the 425 layout; -1 out of range
  static int map[425];
  static bool built = false;
  if (!built) {   // idempotent fill: concurrent first calls write the same values
    for (int i = 0; i < 425; ++i) map[i] = -1;
    for (int depth = 0; depth < 4; ++depth) {
      const int n = 1 << depth, s4 = 16 >> depth;
      for (int cy = 0; cy < n; ++cy)
        for (int cx = 0; cx < n; ++cx) {
          int z = 0;   // raster (4x4 units) -> z-order
          for (int b = 0; b < 4; ++b) z |= (((cx * s4) >> b) & 1) << (2 * b) | (((cy * s4) >> b) & 1) << (2 * b + 1);
          for (int ps = 0; ps < 3; ++ps)
            for (int pi = 0; pi < (ps ? 2 : 1); ++pi) map[hmme_slot_index_amp_off(ps, depth, pi, z)] = hmme_slot_index(ps, depth, pi, z);
        }
    }
    built = true;
  }
  return index_amp_off >= 0 && index_amp_off < 425 ? map[index_amp_off] : -1;
}

int hmme_compact_amp_off(const int16_t* mv593, const uint32_t* sad593, int16_t* mv425, uint32_t* sad425) {
  if (!mv593 || !sad593 || !mv425 || !sad425) return HMME_ERR_ARG;
  for (int i = 0; i < 425; ++i) {
    const int s = hmme_amp_off_slot(i);
    mv425[2 * i] = mv593[2 * s]; mv425[2 * i + 1] = mv593[2 * s + 1];
    sad425[i] = sad593[s];
  }
  return HMME_OK;
}

int hmme_slot_rect(int slot, int* x, int* y, int* w, int* h) {
  if (!x || !y || !w || !h) return HMME_ERR_ARG;
  static const int part_sizes[7] = {0, 1, 2, 4, 5, 6, 7};
  for (int depth = 0; depth < 4; ++depth) {
    const int s = 64 >> depth, n = 1 << depth;
    for (int cy = 0; cy < n; ++cy)
      for (int cx = 0; cx < n; ++cx)
        for (int pi = 0; pi < 7; ++pi)
          for (int idx = 0; idx < 2; ++idx) {
            if (slot_of(part_sizes[pi], depth, idx, cx, cy) != slot) continue;
            int rx = 0, ry = 0, rw = s, rh = s;
            switch (part_sizes[pi]) {   // TComDataCU::getPartIndexAndSize
              case 1: rh = s / 2; ry = idx ? s / 2 : 0; break;
              case 2: rw = s / 2; rx = idx ? s / 2 : 0; break;
              case 4: rh = idx ? 3 * s / 4 : s / 4; ry = idx ? s / 4 : 0; break;
              case 5: rh = idx ? s / 4 : 3 * s / 4; ry = idx ? 3 * s / 4 : 0; break;
              case 6: rw = idx ? 3 * s / 4 : s / 4; rx = idx ? s / 4 : 0; break;
              case 7: rw = idx ? s / 4 : 3 * s / 4; rx = idx ? 3 * s / 4 : 0; break;
              default: break;
            }
            *x = cx * s + rx; *y = cy * s + ry; *w = rw; *h = rh;
            return HMME_OK;
          }
  }
  return HMME_ERR_ARG;
}

int hmme_slot_key(int slot, int* part_size, int* depth, int* part_idx, int* abs_z_idx) {
  if (!part_size || !depth || !part_idx || !abs_z_idx || slot < 0 || slot >= HMME_NUM_CTU_PARTS) return HMME_ERR_ARG;
  static const int part_sizes[7] = {0, 1, 2, 4, 5, 6, 7};
  for (int d = 0; d < 4; ++d) {
    const int n = 1 << d, s4 = 16 >> d;
    for (int cy = 0; cy < n; ++cy)
      for (int cx = 0; cx < n; ++cx)
        for (int pi = 0; pi < 7; ++pi)
          for (int idx = 0; idx < 2; ++idx) {
            if (slot_of(part_sizes[pi], d, idx, cx, cy) != slot) continue;
            int z = 0;   // raster (4x4 units) -> z-order
            for (int b = 0; b < 4; ++b) z |= (((cx * s4) >> b) & 1) << (2 * b) | (((cy * s4) >> b) & 1) << (2 * b + 1);
            *part_size = part_sizes[pi]; *depth = d; *part_idx = idx; *abs_z_idx = z;
            return HMME_OK;
          }
  }
  return HMME_ERR_ARG;
}

// ---- per-CTU drop-in ---------------------------------------------------------------------------------
namespace {
int build_frac_cover(hmme_ctx* ctx);
using frac_fn = void (*)(const RefSet, int, const RefSet, int, const MeJob*, const hmme::FracPrep, int, uint32_t*, const uint16_t*, const int16_t*, uint32_t, int, const hmme::FracWp, int16_t*, uint32_t*);
// One build per (sample width, distortion, weighting) at two waves per SIMD: the 8-bit kernels spill nothing (231 / 237 VGPRs), two
// workgroups per CU.  Round 4's three-wave build of the 8-bit kernel (168 VGPRs + 50 spilled dwords per lane: 104 MB of scratch writes
// per 2160p launch) is gone.
struct FracBuild {
  int wide = 0, had = 0, wp = 0;   // u16 samples (else 8-bit), Hadamard (else SAD), weighted (always on u16 samples)
  int bps() const { return wide ? 2 : 1; }
  int index() const { return (wp ? 2 : wide ? 1 : 0) * 2 + (had ? 1 : 0); }
};
inline frac_fn frac_kernel(FracBuild b) {
  static const frac_fn fns[6] = {hmme::me_frac_kernel<0, 1, 0, 2>, hmme::me_frac_kernel<1, 1, 0, 2>, hmme::me_frac_kernel<0, 2, 0>, hmme::me_frac_kernel<1, 2, 0>,
                                 hmme::me_frac_kernel<0, 2, 1>, hmme::me_frac_kernel<1, 2, 1>};
  return fns[b.index()];
}
// more than 64 KiB of dynamic LDS: opt in once per kernel and context
int frac_lds_optin(hmme_ctx* ctx, FracBuild b) {
  bool& done = ctx->frac_lds_optin[b.index()];
  if (done) return HMME_OK;
  const size_t bytes = hmme::frac_lds_bytes(b.bps());
  if (bytes > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)frac_kernel(b), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return fail(ctx, HMME_ERR_DEVICE, "hipFuncSetAttribute(me_frac_kernel, %zu bytes of LDS) -> %s", bytes, hipGetErrorString(e));
  }
  done = true;
  return HMME_OK;
}
const hmme::FracWp kNoWp = {0.f, 0.f, 0.f};
const hmme::FracPrep kNoPrep = {nullptr, 1u << 16, 0, 0};
// workgroups of a refinement launch: one per job, dealt from the end of the job table (me_frac_kernel).  HMME_FRAC_GRID=<n> launches n
// workgroups that take job after job from a counter instead, HMME_FRAC_GRID=-1 as many of those as the chip holds at a time (the
// runtime's occupancy figure for this kernel with its LDS block x the CUs): round 4's intermediate launch, kept for A/B runs -- once
// both orders ran last-first it was the slower one on every content (profiles/r04g_frac_grid_both_last_first.txt)
int frac_grid(hmme_ctx* ctx, FracBuild b, int jobs) {
  const int forced = knobs().frac_grid;
  if (forced == 0) return jobs;
  int grid = forced;
  if (forced < 0) {
    int& per_cu = ctx->frac_wg_per_cu[b.index()];
    if (per_cu == 0) {
      int n = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)frac_kernel(b), hmme::frac_threads(b.bps()), hmme::frac_lds_bytes(b.bps())) != hipSuccess || n < 1) {
        (void)hipGetLastError();
        n = 2;
      }
      per_cu = n;
      if (knobs().trace) fprintf(stderr, "hmme: me_frac_kernel<%d, %d, %d>: %d workgroups per CU, %d CUs\n", b.had ? 1 : 0, b.bps(), b.wp ? 1 : 0, n, ctx->num_cus);
    }
    grid = per_cu * ctx->num_cus;
  }
  return grid < jobs ? grid : jobs;
}

// host-side packing of the call block, one picture row at a time; separate reduction and narrowing loops so that the compiler
// vectorises both (the reference copies the same window sample by sample, TEncOpenCL.cpp:275-277)
inline void row_minmax(const int16_t* __restrict__ s, int n, int& lo, int& hi) {
  int16_t l = (int16_t)(lo < -32768 ? -32768 : lo), h = (int16_t)(hi > 32767 ? 32767 : hi);
  for (int x = 0; x < n; ++x) { l = s[x] < l ? s[x] : l; h = s[x] > h ? s[x] : h; }
  lo = l; hi = h;
}
inline void row_pack8(const int16_t* __restrict__ s, int n, uint8_t* __restrict__ d) {
  for (int x = 0; x < n; ++x) d[x] = (uint8_t)s[x];
}
inline void row_pack16(const int16_t* __restrict__ s, int n, int bias, uint16_t* __restrict__ d) {
  for (int x = 0; x < n; ++x) d[x] = (uint16_t)(s[x] + bias);
}

// a refusal: its message into msg, its code back
static __attribute__((format(printf, 4, 5))) int refuse(char* msg, size_t n, int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(msg, n, fmt, ap);
  va_end(ap);
  return code;
}

// The range rule of a weighted reference, for the per-CTU calls (on the ranges they scan: ctu_plan_window) and the picture-level ones (on
// nominal ranges: weight_eval) alike.  Reference samples in [rlo, rhi] under weight wp, compared with a block in [blo, bhi], the sums
// shifted by cost_shift (the kernels' shift_bd - 8): the weighted range and the bias that keeps block and weighted samples unsigned,
// or the refusal.
struct WeightRange { long wlo = 0, whi = 0; int bias = 0; };
static int weight_range(const hmme_weight* wp, long rlo, long rhi, long blo, long bhi, int cost_shift, bool refine, WeightRange* out, char* msg, size_t n) {
  const long a = (((long)wp->w0 * rlo + wp->round) >> wp->shift) + wp->offset, b = (((long)wp->w0 * rhi + wp->round) >> wp->shift) + wp->offset;   // monotonic between
  const long wlo = std::min(a, b), whi = std::max(a, b);
  // HM keeps the weighted sample in a Pel (`const Pel pred`, TComRdCostWeightPrediction.cpp:79): beyond int16 its arithmetic wraps,
  // which nothing here reproduces -- such a call goes back to the caller
  if (wlo < -32768 || whi > 32767) return refuse(msg, n, HMME_ERR_UNSUPPORTED, "weighted prediction reaches %ld..%ld, beyond a Pel", wlo, whi);
  const long bias = std::max(0L, -std::min(wlo, blo));
  // cannot fire for a block within [-maxv, 2 * maxv] of at most 12 bits (bias <= 32768 and whi <= 32767, 8190 + 4095 otherwise); kept as
  // the statement of what the u16 staging needs
  if (std::max(whi, bhi) + bias > 65535) return refuse(msg, n, HMME_ERR_UNSUPPORTED, "weighted prediction: samples span more than 16 bits");
  // the sums of a weighted search must fit the cost field like any other (the weighted window may be far from the block)
  const long span = std::max(bhi - wlo, whi - blo);   // largest |block - weighted sample| the two ranges admit
  if (((4096 * span) >> cost_shift) + 65535 >= (long)hmme::kInvCost16)
    return refuse(msg, n, HMME_ERR_UNSUPPORTED, "weighted SADs of this block could reach %ld: beyond the cost field", 4096 * span);
  // the refinement's Hadamard sums are exact in fp32 below 2^24: 64 coefficients of up to 64 * span each
  if (refine && 4096 * span >= (1L << 24))
    return refuse(msg, n, HMME_ERR_UNSUPPORTED, "weighted refinement: sample differences up to %ld exceed what the Hadamard sums hold exactly", span);
  *out = {wlo, whi, (int)bias};
  return HMME_OK;
}
// frac_wp: weight w on current samples staged with `bias` -- org_sub takes the bias off again, with the weight's offset; null: the weight is 1
inline hmme::FracWp frac_wp(const hmme_weight* w, int bias) {
  if (!w) return hmme::FracWp{1.f, 0.f, (float)bias};
  return hmme::FracWp{std::ldexp((float)w->w0, -w->shift), std::ldexp((float)w->round, -w->shift), (float)(bias + w->offset)};
}

// One (CTU, reference) call: search (out_mv / out_sad), refinement of the winners or of the caller's integer MVs (out_qmv / out_cost), or
// both.  ctu_call below is the sequence of: the refusals that need no sample (ctu_arg_check), the plan -- pure host arithmetic over the
// parameters, the weight and the four scanned numbers, in two stages (ctu_plan_block, ctu_plan_window) --, packing (ctu_pack), the
// launches (ctu_stage, ctu_launch_search, ctu_launch_refine), the wait and the copy-out (ctu_finish).  hmme_test_ctu_plan shows the
// first two to the CPU tests.  The order of the refusals is part of the boundary (tests/ctu_refusal_cases.py): TEncOpenCL retries on
// HMME_ERR_RANGE alone.
enum : int { kCtuSearch = HMME_TEST_CTU_SEARCH, kCtuRefine = HMME_TEST_CTU_REFINE, kCtuHadamard = HMME_TEST_CTU_HADAMARD };   // a call's mode

// null_arg: one of the call's pointers is null, p included
static int ctu_arg_check(const hmme_search_params* p, const hmme_weight* wp, bool null_arg, char* msg, size_t n) {
  if (wp && (wp->shift < 0 || wp->shift > 15)) return refuse(msg, n, HMME_ERR_ARG, "weighted prediction: shift %d outside 0..15", wp->shift);
  if (null_arg) return refuse(msg, n, HMME_ERR_ARG, "hmme_search_ctu: null argument");
  if (p->bit_depth < 8 || p->bit_depth > 12) return refuse(msg, n, HMME_ERR_UNSUPPORTED, "bit depth %d outside 8..12", p->bit_depth);
  // MeJob carries the window and the predictor as int16 (what TComMv holds, TComMv.h:51-55): anything wider would address
  // the staged window at a truncated offset
  const int v[6] = {p->lt_x, p->lt_y, p->rb_x, p->rb_y, p->pred_x, p->pred_y};
  for (int i = 0; i < 6; ++i)
    if (v[i] < -32768 || v[i] > 32767) return refuse(msg, n, HMME_ERR_ARG, "hmme_search_ctu: window / predictor component %d outside int16", v[i]);
  return HMME_OK;
}

struct CtuPlan {
  int mode = 0, lo = 0, hi = 0;                       // what the call does; the range of its block
  int wx = 0, wy = 0, halo = 0, rows = 0, cols = 0;   // candidates; the staged window: `halo` samples on every side, rows x cols in all
  bool wide = false, origin = false;                  // the 16-bit kernels on u16 samples; the block is a bi-prediction origin
  int bias = 0, shift_bd = 8;                         // added to the staged samples; the kernels shift their sums by (shift_bd - 8)
  FracBuild build;
  hmme::FracWp fw = kNoWp;
  MeJob job;                                          // the whole window
  int n_wg = 0, pdw = 0, smax = 0, tile_tasks[4] = {0, 0, 0, 0};   // the deal; 8-bit: tasks of tile ty * 2 + tx
  int bps() const { return wide ? 2 : 1; }
};

// one CTU alone would keep a few of the 256 CUs busy: its work is dealt to up to 64 workgroups (task ranges and window tiles on
// the 8-bit path, strips of candidate rows on the 16-bit path) that merge through the 64-bit atomicMin table
static void ctu_deal(CtuPlan* pl, MeJob16* js) {
  const MeJob& job = pl->job;
  if (!(pl->mode & kCtuSearch)) {
    js[0].j = job; js[0].job = 0; js[0].y0 = js[0].y1 = 0;
  } else if (!pl->wide) {
    // windows beyond 129 x 129 candidates: up to 2 x 2 tiles (tile (0,0) first: finalize decodes against its top-left)
    const int tiles_x = (pl->wx + hmme::kTileStep - 1) / hmme::kTileStep, tiles_y = (pl->wy + hmme::kTileStep - 1) / hmme::kTileStep;
    const int per_tile = kCallMaxJobs / (tiles_x * tiles_y);
    for (int ty = 0; ty < tiles_y; ++ty)
      for (int tx = 0; tx < tiles_x; ++tx) {
        const MeJob sub = hmme::me_tile_job(job, tx, ty);
        const int nt = pl->tile_tasks[ty * 2 + tx] = hmme::me_num_tasks(sub.rb_x - sub.lt_x + 1, sub.rb_y - sub.lt_y + 1);
        const int parts = std::max(1, std::min(per_tile, (nt + 3) / 4));   // 4 tasks = one per wave
        for (int i = 0; i < parts; ++i, ++pl->n_wg) {
          MeJob16& w = js[pl->n_wg];
          w.j = sub; w.job = 0 | tx << 30 | ty << 29;
          w.y0 = (int16_t)((long)nt * i / parts); w.y1 = (int16_t)((long)nt * (i + 1) / parts);
        }
      }
  } else {
    pl->pdw = pick_pdw16(pl->wx);
    // at least as many strips as the LDS needs (never more than kCallMaxJobs: the static_assert beside strips_for), and enough of them
    // to spread the CTU over the chip: a strip is >= 4 candidate rows (each also stages the 63 rows below it)
    pl->n_wg = std::max(strips_for(pl->pdw, pl->wy), std::min(kCallMaxJobs, (pl->wy + 3) / 4));
    for (int i = 0; i < pl->n_wg; ++i) {
      js[i].j = job; js[i].job = 0;
      js[i].y0 = (int16_t)((long)pl->wy * i / pl->n_wg); js[i].y1 = (int16_t)((long)pl->wy * (i + 1) / pl->n_wg);
      pl->smax = std::max(pl->smax, js[i].y1 - js[i].y0);
    }
  }
}

// The plan, first stage: what the parameters and the range [lo, hi] of the block decide -- sample width, origin bias, window geometry,
// the refinement's build and the deal (js: kCallMaxJobs entries).  Pure arithmetic: no context, no device.
static int ctu_plan_block(const hmme_search_params* p, bool weighted, int mode, int sr_max, int lo, int hi, CtuPlan* pl, MeJob16* js, char* msg, size_t n) {
  const int maxv = (1 << p->bit_depth) - 1;
  *pl = CtuPlan{};
  pl->mode = mode; pl->lo = lo; pl->hi = hi;
  // samples outside [0, maxv] are the bi-prediction origin 2*org - pred_other (reference TEncSearch.cpp:3702-3712,
  // TComYuv::removeHighFreq TComYuv.cpp:409-440, unclipped).  They stay exact: the 16-bit kernel runs on samples
  // biased by 2^bitDepth (|a - b| is unchanged), so the kernel is picked after looking at the data.
  if (lo < -maxv || hi > 2 * maxv)
    return refuse(msg, n, HMME_ERR_RANGE, "hmme_search_ctu: current-block sample outside [%d, %d] (bit depth %d)", -maxv, 2 * maxv, p->bit_depth);
  pl->wx = p->rb_x - p->lt_x + 1; pl->wy = p->rb_y - p->lt_y + 1;
  if (pl->wx < 1 || pl->wy < 1 || pl->wx > 2 * sr_max + 1 || pl->wy > 2 * sr_max + 1)
    return refuse(msg, n, HMME_ERR_ARG, "window %dx%d outside 1..%d", pl->wx, pl->wy, 2 * sr_max + 1);
  pl->origin = lo < 0 || hi > maxv;
  pl->wide = p->bit_depth > 8 || pl->origin || weighted;
  // xPatternSearchFracDIF on 2*org - pred_other (the bBi pass, TEncSearch.cpp:3798 with bBi): the refinement kernel runs on the same
  // biased u16 staging as the search; the bias passes HM's interpolation exactly and shifts its clip bounds (me_kernels.hpp, the
  // evaluation of one work item).  A weighted call's bias is chosen with its window's range (ctu_plan_window).
  pl->bias = pl->origin ? (1 << p->bit_depth) : 0;
  pl->shift_bd = p->shift_free ? 8 : p->bit_depth;
  pl->halo = (mode & kCtuRefine) ? kRefineHalo : 0;   // what the 8-tap interpolation reaches beyond the window
  pl->rows = pl->wy + 63 + 2 * pl->halo; pl->cols = pl->wx + 63 + 2 * pl->halo;
  pl->build = FracBuild{pl->wide ? 1 : 0, (mode & kCtuHadamard) ? 1 : 0, weighted ? 1 : 0};
  pl->job.ctu_x = 0; pl->job.ctu_y = 0;
  pl->job.lt_x = (int16_t)p->lt_x; pl->job.lt_y = (int16_t)p->lt_y; pl->job.rb_x = (int16_t)p->rb_x; pl->job.rb_y = (int16_t)p->rb_y;
  pl->job.pred_x = (int16_t)p->pred_x; pl->job.pred_y = (int16_t)p->pred_y;
  ctu_deal(pl, js);
  return HMME_OK;
}

// The plan, second stage: what the range [vlo, vhi] of the staged window decides.  A weighted call comes here before it packs (block
// and weighted window share a bias), any other after: its window is scanned in the loop that packs it.
static int ctu_plan_window(const hmme_search_params* p, const hmme_weight* wp, int vlo, int vhi, CtuPlan* pl, char* msg, size_t n) {
  const int maxv = (1 << p->bit_depth) - 1;
  if (vlo < 0 || vhi > maxv) return refuse(msg, n, HMME_ERR_RANGE, "hmme_search_ctu: reference sample outside [0,%d] for bit depth %d", maxv, p->bit_depth);
  if (wp) {
    WeightRange wr;
    const int rc = weight_range(wp, vlo, vhi, pl->lo, pl->hi, pl->shift_bd - 8, (pl->mode & kCtuRefine) != 0, &wr, msg, n);
    if (rc) return rc;
    // the interpolated prediction is weighted sample by sample (me_frac_eval0 / me_frac_eval1, FracWp); the current samples carry `bias`, the raw window none
    pl->bias = wr.bias;
    pl->fw = frac_wp(wp, wr.bias);
  }
  // unshifted sums must fit the 24-bit cost field of the 16-bit kernel's keys (me_kernels.hpp kInvCost16).  The bound is taken
  // from the samples of THIS call (both scans are made anyway): no |cur - ref| exceeds max(hi - vlo, vhi - lo), so any content whose
  // 64x64 sum cannot reach the marker is searched, whatever the nominal bit depth says (10-bit bi-prediction origins nominally
  // reach 4096 * 2046, real ones stay far below)
  if (p->shift_free && pl->wide) {
    const long span = std::max<long>((long)pl->hi - vlo, (long)vhi - pl->lo);
    if (4096 * span + 65535 >= (long)hmme::kInvCost16)
      return refuse(msg, n, HMME_ERR_UNSUPPORTED, "shift-free SADs of this block could reach %ld (sample difference up to %ld at bit depth %d%s): beyond the cost field",
                    4096 * span, span, p->bit_depth, pl->origin ? ", bi-prediction origin" : "");
  }
  return HMME_OK;
}

// Block, window and the refinement's inputs into the pinned call block (the reference copies the same window with a scalar CPU loop,
// TEncOpenCL.cpp:275-277); 1 byte per sample on the 8-bit path, 2 otherwise.  win_range: where the window's range goes, taken in the
// same pass (null: scanned before, the weighted call -- its window goes up as it is and is weighted on the device).
static void ctu_pack(hmme_ctx* ctx, const CtuPlan& pl, const int16_t* ctu, int ctu_stride, const int16_t* src, int ref_stride, const int16_t* int_mv, int* win_range) {
  uint8_t* h_ctu = ctx->h_call + kCallCtu;
  uint8_t* h_win = ctx->h_call + kCallWin;
  // the plan's numbers as locals: the byte stores below may alias anything the compiler cannot see the end of
  const bool wide = pl.wide, scan = win_range != nullptr;
  const int rows = pl.rows, cols = pl.cols, bps = pl.bps(), bias = pl.bias, win_bias = pl.build.wp ? 0 : pl.bias;
  int vlo = 32767, vhi = -32768;
  for (int y = 0; y < 64; ++y) {
    if (wide) row_pack16(ctu + (long)y * ctu_stride, 64, bias, (uint16_t*)h_ctu + y * 64);
    else row_pack8(ctu + (long)y * ctu_stride, 64, h_ctu + y * 64);
  }
  for (int y = 0; y < rows; ++y) {
    uint8_t* row = h_win + (size_t)y * kWinPitch;
    const int16_t* srow = src + (long)y * ref_stride;
    if (scan) row_minmax(srow, cols, vlo, vhi);
    if (wide) row_pack16(srow, cols, win_bias, (uint16_t*)row);
    else row_pack8(srow, cols, row);
    std::memset(row + cols * bps, 0, 16);   // the kernels stage whole dwords past the last sample
  }
  if (win_range) { win_range[0] = vlo; win_range[1] = vhi; }
  if (int_mv) std::memcpy(ctx->h_call + kCallImv, int_mv, sizeof(int16_t) * 2 * HMME_NUM_CTU_PARTS);
  std::memcpy(ctx->h_call + kCallFracJob, &pl.job, sizeof pl.job);
}

// the kernels address ref(ctu + lt): the base is biased so that (lt_x, lt_y) lands on the first sample of the window copy at `win`
inline const uint8_t* ctu_ref_base(const uint8_t* win, const CtuPlan& pl) {
  return win - (long)(pl.job.lt_y - pl.halo) * kWinPitch - (long)(pl.job.lt_x - pl.halo) * pl.bps();
}

// the call block to the device; a weighted search runs on a weighted copy of the window, the raw one stays where it is for the refinement's interpolation
static int ctu_stage(hmme_ctx* ctx, const CtuPlan& pl, const hmme_weight* wp) {
  hipStream_t s = ctx->stream;
  const int n16 = (int)((kCallWin + (size_t)pl.rows * kWinPitch + 64 + 15) / 16);
  hipLaunchKernelGGL(hmme::me_stage_call_kernel, dim3((n16 + 255) / 256), dim3(256), 0, s, (const uint4*)ctx->h_call_dev, (uint4*)ctx->d_call(), n16);
  HIP_TRY(ctx, hipGetLastError());
  if (!wp || !(pl.mode & kCtuSearch)) return HMME_OK;
  bool fresh;   // cleared once: rows below a call's window hold zeros or an earlier call's samples, never what the allocator left
  const int erc = ensure(ctx, ctx->buf[kWwin], (size_t)kWinRows * kWinPitch + 64, 0, &fresh);
  if (erc) return erc;
  if (fresh) HIP_TRY(ctx, hipMemsetAsync(ctx->buf[kWwin].p, 0, (size_t)kWinRows * kWinPitch + 64, s));
  hipLaunchKernelGGL(hmme::me_weight_window_kernel, dim3((pl.rows * (pl.cols + 8) + 255) / 256), dim3(256), 0, s, (const uint8_t*)(ctx->d_call() + kCallWin), ctx->buf[kWwin].as<uint8_t>(),
                     (int)kWinPitch, pl.rows, pl.cols, wp->w0, wp->round, wp->shift, wp->offset + pl.bias);
  HIP_TRY(ctx, hipGetLastError());
  return HMME_OK;
}

// the 4.7 KB of results go straight into pinned host memory (mapped into the device's address space): no download step
static int ctu_launch_search(hmme_ctx* ctx, const CtuPlan& pl, int fen, bool weighted, uint32_t seq) {
  hipStream_t s = ctx->stream;
  const uint8_t* win = weighted ? ctx->buf[kWwin].as<uint8_t>() : ctx->d_call() + kCallWin;
  const MeJob16* d_js = (const MeJob16*)(ctx->d_call() + kCallJobs);
  const int* d_first = (const int*)(ctx->d_call() + kCallFirst);
  unsigned long long* d_best1 = (unsigned long long*)(ctx->d_call() + kCallBest);
  int16_t* d_mv1 = (int16_t*)(ctx->d_res + kResMv);
  uint32_t* d_sad1 = (uint32_t*)(ctx->d_res + kResSad);
  int rc;
  if (!pl.wide)
    rc = launch_search8_split(ctx, one_ref(ctx->d_call() + kCallCtu), 1, one_ref(ctu_ref_base(win, pl)), kWinPitch, d_js, d_first, 1, pl.n_wg, fen, d_mv1, d_sad1, s, d_best1, false);
  else
    rc = launch_search16(ctx, one_ref(ctx->d_call() + kCallCtu), 1, one_ref(ctu_ref_base(win, pl)), kWinPitch, d_js, d_first, 1, pl.n_wg, pl.pdw, pl.smax, weighted ? 0 : fen,   // xGetSADw reads every row
                         pl.shift_bd, d_mv1, d_sad1, s, d_best1, false);
  if (rc) return rc;
  hipLaunchKernelGGL(hmme::me_finalize1_kernel, dim3(1), dim3(640), 0, s, d_best1, d_js, ctx->lambda_q16, d_mv1, d_sad1,
                     (volatile uint32_t*)(ctx->d_res + kResDone), seq);
  HIP_TRY(ctx, hipGetLastError());
  return HMME_OK;
}

// xPatternSearchFracDIF for the 593 slots on the block and window that are staged anyway: one more workgroup-sized kernel,
// its input the integer tables the finalize kernel just wrote (or the caller's), its output in the same pinned block
static int ctu_launch_refine(hmme_ctx* ctx, const CtuPlan& pl, int bit_depth, uint32_t seq) {
  hipStream_t s = ctx->stream;
  int rc = build_frac_cover(ctx);
  if (rc) return rc;
  const int16_t* d_imv = (pl.mode & kCtuSearch) ? (const int16_t*)(ctx->d_res + kResMv) : (const int16_t*)(ctx->d_call() + kCallImv);
  rc = frac_lds_optin(ctx, pl.build);
  if (rc) return rc;
  hipLaunchKernelGGL(frac_kernel(pl.build), dim3(1), dim3(hmme::frac_threads(pl.bps())), hmme::frac_lds_bytes(pl.bps()), s, one_ref(ctx->d_call() + kCallCtu),
                     64 * pl.bps(), one_ref(ctu_ref_base(ctx->d_call() + kCallWin, pl)), kWinPitch, (const MeJob*)(ctx->d_call() + kCallFracJob), kNoPrep, 1, (uint32_t*)nullptr,
                     ctx->buf[kFracCover].as<uint16_t>(), d_imv, ctx->lambda_q16, bit_depth | ((pl.origin && !pl.build.wp) ? 0x100 : 0), pl.fw,
                     (int16_t*)(ctx->d_res + kResQmv), (uint32_t*)(ctx->d_res + kResCost));
  HIP_TRY(ctx, hipGetLastError());
  hipLaunchKernelGGL(hmme::me_publish_kernel, dim3(1), dim3(1), 0, s, (volatile uint32_t*)(ctx->d_res + kResDone2), seq);
  HIP_TRY(ctx, hipGetLastError());
  return HMME_OK;
}

// the caller blocks on this call anyway (TEncSearch.cpp:3749-3758): poll the completion word for a while instead of paying the
// interrupt wake-up of hipStreamSynchronize, then fall back to it (a faulted kernel never publishes); then the tables to the caller
static int ctu_finish(hmme_ctx* ctx, int mode, uint32_t seq, int16_t* out_mv, uint32_t* out_sad, int16_t* out_qmv, uint32_t* out_cost) {
  volatile uint32_t* done = (volatile uint32_t*)(ctx->h_res + ((mode & kCtuRefine) ? kResDone2 : kResDone));
  for (int spin = 0; *done != seq && spin < 200000; ++spin) __builtin_ia32_pause();
  if (*done != seq) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (*done != seq) return fail(ctx, HMME_ERR_DEVICE, "hmme_search_ctu: the device did not publish results");
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  if (mode & kCtuSearch) {
    std::memcpy(out_mv, ctx->h_res + kResMv, sizeof(int16_t) * 2 * HMME_NUM_CTU_PARTS);
    std::memcpy(out_sad, ctx->h_res + kResSad, sizeof(uint32_t) * HMME_NUM_CTU_PARTS);
  }
  if (mode & kCtuRefine) {
    std::memcpy(out_qmv, ctx->h_res + kResQmv, sizeof(int16_t) * 2 * HMME_NUM_CTU_PARTS);
    std::memcpy(out_cost, ctx->h_res + kResCost, sizeof(uint32_t) * HMME_NUM_CTU_PARTS);
  }
  return HMME_OK;
}

static int ctu_call(hmme_ctx* ctx, const int16_t* ctu, int ctu_stride, const int16_t* ref0, int ref_stride, const hmme_search_params* p, int mode,
             const int16_t* int_mv, int16_t* out_mv, uint32_t* out_sad, int16_t* out_qmv, uint32_t* out_cost, const hmme_weight* wp = nullptr) {
  if (!ctx) return HMME_ERR_ARG;
  const bool search = mode & kCtuSearch, refine = mode & kCtuRefine;
  char why[256];
  int rc = ctu_arg_check(p, wp, !ctu || !ref0 || !p || (search && (!out_mv || !out_sad)) || (refine && (!out_qmv || !out_cost)) || (!search && !int_mv), why, sizeof why);
  if (rc) return fail(ctx, rc, "%s", why);
  int lo = 32767, hi = -32768, win[2] = {32767, -32768};
  for (int y = 0; y < 64; ++y) row_minmax(ctu + (long)y * ctu_stride, 64, lo, hi);
  CtuPlan pl;
  rc = ctu_plan_block(p, wp != nullptr, mode, ctx->sr_max, lo, hi, &pl, (MeJob16*)(ctx->h_call + kCallJobs), why, sizeof why);
  if (rc) return fail(ctx, rc, "%s", why);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int16_t* src = ref0 + (long)(p->lt_y - pl.halo) * ref_stride + (p->lt_x - pl.halo);
  if (wp) {   // scanned once before the bias is chosen; every other window in the loop that packs it
    for (int y = 0; y < pl.rows; ++y) row_minmax(src + (long)y * ref_stride, pl.cols, win[0], win[1]);
    rc = ctu_plan_window(p, wp, win[0], win[1], &pl, why, sizeof why);
  }
  if (!rc) ctu_pack(ctx, pl, ctu, ctu_stride, src, ref_stride, search ? nullptr : int_mv, wp ? nullptr : win);
  if (!rc && !wp) rc = ctu_plan_window(p, wp, win[0], win[1], &pl, why, sizeof why);
  if (rc) return fail(ctx, rc, "%s", why);
  const uint32_t seq = ++ctx->call_seq ? ctx->call_seq : ++ctx->call_seq;   // never 0, the words' initial value
  rc = ctu_stage(ctx, pl, wp);
  if (!rc && search) rc = ctu_launch_search(ctx, pl, p->fen, wp != nullptr, seq);
  if (!rc && refine) rc = ctu_launch_refine(ctx, pl, p->bit_depth, seq);
  return rc ? rc : ctu_finish(ctx, mode, seq, out_mv, out_sad, out_qmv, out_cost);
}
}  // namespace

int hmme_test_ctu_plan(int sr_max, const hmme_search_params* p, int mode, const hmme_weight* wp, const int* range, int* out, float* out_fw, int16_t* out_wg, char* msg, int msg_len) {
  char why[256];
  why[0] = 0;
  if (!p || !range || !out || !out_fw || !out_wg || sr_max < 1 || sr_max > HMME_MAX_SEARCH_RANGE || !(mode & (kCtuSearch | kCtuRefine)) ||
      ((mode & kCtuHadamard) && !(mode & kCtuRefine)))
    return HMME_ERR_ARG;
  CtuPlan pl;
  MeJob16 js[kCallMaxJobs];
  int rc = ctu_arg_check(p, wp, false, why, sizeof why);
  if (!rc) rc = ctu_plan_block(p, wp != nullptr, mode, sr_max, range[0], range[1], &pl, js, why, sizeof why);
  if (!rc) rc = ctu_plan_window(p, wp, range[2], range[3], &pl, why, sizeof why);
  if (msg && msg_len > 0) snprintf(msg, (size_t)msg_len, "%s", why);
  if (rc) return rc;
  const int scalars[17] = {pl.wide, pl.bias, pl.origin, pl.shift_bd, pl.halo, pl.rows, pl.cols, pl.n_wg, pl.pdw, pl.smax, pl.build.wide, pl.build.had, pl.build.wp,
                           pl.tile_tasks[0], pl.tile_tasks[1], pl.tile_tasks[2], pl.tile_tasks[3]};
  std::memcpy(out, scalars, sizeof scalars);
  out_fw[0] = pl.fw.ws; out_fw[1] = pl.fw.rs; out_fw[2] = pl.fw.org_sub;
  for (int i = 0; i < pl.n_wg; ++i) {
    const int16_t wg[8] = {js[i].j.lt_x, js[i].j.lt_y, js[i].j.rb_x, js[i].j.rb_y, (int16_t)((js[i].job >> 30) & 1), (int16_t)((js[i].job >> 29) & 1), js[i].y0, js[i].y1};
    std::memcpy(out_wg + 8 * i, wg, sizeof wg);
  }
  return HMME_OK;
}

static inline int refine_mode(int use_hadamard) { return kCtuRefine | (use_hadamard ? kCtuHadamard : 0); }

int hmme_search_ctu(hmme_ctx* ctx, const int16_t* ctu, int ctu_stride, const int16_t* ref0, int ref_stride,
                    const hmme_search_params* p, int16_t* out_mv, uint32_t* out_sad) {
  return ctu_call(ctx, ctu, ctu_stride, ref0, ref_stride, p, kCtuSearch, nullptr, out_mv, out_sad, nullptr, nullptr);
}

int hmme_search_ctu_w(hmme_ctx* ctx, const int16_t* ctu, int ctu_stride, const int16_t* ref0, int ref_stride,
                      const hmme_search_params* p, const hmme_weight* wp, int16_t* out_mv, uint32_t* out_sad) {
  if (ctx && !wp) return fail(ctx, HMME_ERR_ARG, "hmme_search_ctu_w: null weight");
  return ctu_call(ctx, ctu, ctu_stride, ref0, ref_stride, p, kCtuSearch, nullptr, out_mv, out_sad, nullptr, nullptr, wp);
}

int hmme_search_refine_ctu_w(hmme_ctx* ctx, const int16_t* ctu, int ctu_stride, const int16_t* ref0, int ref_stride, const hmme_search_params* p,
                             const hmme_weight* wp, int use_hadamard, int16_t* out_mv, uint32_t* out_sad, int16_t* out_qmv, uint32_t* out_cost) {
  if (ctx && !wp) return fail(ctx, HMME_ERR_ARG, "hmme_search_refine_ctu_w: null weight");
  return ctu_call(ctx, ctu, ctu_stride, ref0, ref_stride, p, kCtuSearch | refine_mode(use_hadamard), nullptr, out_mv, out_sad, out_qmv, out_cost, wp);
}

int hmme_search_refine_ctu(hmme_ctx* ctx, const int16_t* ctu, int ctu_stride, const int16_t* ref0, int ref_stride, const hmme_search_params* p,
                           int use_hadamard, int16_t* out_mv, uint32_t* out_sad, int16_t* out_qmv, uint32_t* out_cost) {
  return ctu_call(ctx, ctu, ctu_stride, ref0, ref_stride, p, kCtuSearch | refine_mode(use_hadamard), nullptr, out_mv, out_sad, out_qmv, out_cost);
}

int hmme_refine_ctu(hmme_ctx* ctx, const int16_t* ctu, int ctu_stride, const int16_t* ref0, int ref_stride, const hmme_search_params* p,
                    const int16_t* int_mv, int use_hadamard, int16_t* out_qmv, uint32_t* out_cost) {
  return ctu_call(ctx, ctu, ctu_stride, ref0, ref_stride, p, refine_mode(use_hadamard), int_mv, nullptr, nullptr, out_qmv, out_cost);
}

int hmme_refine_ctu_w(hmme_ctx* ctx, const int16_t* ctu, int ctu_stride, const int16_t* ref0, int ref_stride, const hmme_search_params* p,
                      const hmme_weight* wp, const int16_t* int_mv, int use_hadamard, int16_t* out_qmv, uint32_t* out_cost) {
  if (ctx && !wp) return fail(ctx, HMME_ERR_ARG, "hmme_refine_ctu_w: null weight");
  return ctu_call(ctx, ctu, ctu_stride, ref0, ref_stride, p, refine_mode(use_hadamard), int_mv, nullptr, nullptr, out_qmv, out_cost, wp);
}

// ---- planes ----------------------------------------------------------------------------------------------
int hmme_plane_create_ex(hmme_ctx* ctx, int width, int height, int bit_depth, hmme_plane** out) {
  if (!ctx) return HMME_ERR_ARG;
  if (!out || width < 8 || height < 8 || width > 16384 || height > 16384) return fail(ctx, HMME_ERR_ARG, "hmme_plane_create(%d, %d)", width, height);
  if (bit_depth < 8 || bit_depth > 12) return fail(ctx, HMME_ERR_UNSUPPORTED, "bit depth %d outside 8..12", bit_depth);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hmme_plane* pl = new hmme_plane;
  pl->ctx = ctx; pl->width = width; pl->height = height;
  pl->bit_depth = bit_depth; pl->bps = bit_depth > 8 ? 2 : 1;
  pl->pitch = ((width + 2 * kMarginX) * pl->bps + 255) & ~255;
  pl->rows = height + 2 * kMarginY;
  pl->ctus_x = (width + 63) / 64; pl->n_ctu = hmme_num_ctus(width, height);
  hipError_t e = hipMalloc(&pl->d_data, (size_t)pl->pitch * (pl->rows + 1));
  if (e == hipSuccess && (e = hipMalloc(&pl->d_blocks, (size_t)pl->n_ctu * hmme::kBlkBytes8 * pl->bps)) != hipSuccess) hipFree(pl->d_data);
  if (e == hipSuccess && (e = hipEventCreateWithFlags(&pl->filled, hipEventDisableTiming)) != hipSuccess) { hipFree(pl->d_data); hipFree(pl->d_blocks); }
  if (e != hipSuccess) { delete pl; return fail(ctx, HMME_ERR_NOMEM, "plane allocation: %s", hipGetErrorString(e)); }
  *out = pl;
  return HMME_OK;
}
int hmme_plane_create(hmme_ctx* ctx, int width, int height, hmme_plane** out) { return hmme_plane_create_ex(ctx, width, height, 8, out); }

void hmme_plane_destroy(hmme_plane* pl) {
  if (!pl) return;
  hipSetDevice(pl->ctx->device);
  if (pl->fill_pending) hipEventSynchronize(pl->filled);   // a fill or a search still in flight must not outlive the buffer
  if (pl->read_pending) hipEventSynchronize(pl->read_done);
  if (pl->filled) hipEventDestroy(pl->filled);
  hipFree(pl->d_data);
  hipFree(pl->d_blocks);
  hipFree(pl->stage.p);
  delete pl;
}

int hmme_plane_width(const hmme_plane* pl) { return pl ? pl->width : 0; }
int hmme_plane_height(const hmme_plane* pl) { return pl ? pl->height : 0; }
int hmme_plane_bit_depth(const hmme_plane* pl) { return pl ? pl->bit_depth : 0; }

int hmme_plane_upload_pel(hmme_plane* pl, const int16_t* origin, int stride) { return plane_upload<int16_t>(pl, origin, stride, nullptr, true); }
int hmme_plane_upload_u8(hmme_plane* pl, const uint8_t* origin, int stride) { return plane_upload<uint8_t>(pl, origin, stride, nullptr, true); }

int hmme_plane_upload_async(hmme_plane* pl, const void* origin, int stride, int sample_bytes, void* stream) {
  if (!pl) return HMME_ERR_ARG;
  if (sample_bytes == 1) return plane_upload<uint8_t>(pl, (const uint8_t*)origin, stride, (hipStream_t)stream, false);
  // 16-bit samples (HM's Pel, or the unsigned words of a 16-bit YUV file: anything beyond the bit depth reads as negative or too large)
  if (sample_bytes == 2) return plane_upload<int16_t>(pl, (const int16_t*)origin, stride, (hipStream_t)stream, false);
  return fail(pl->ctx, HMME_ERR_ARG, "hmme_plane_upload_async: sample_bytes %d (1 or 2)", sample_bytes);
}

int hmme_upload_status(hmme_ctx* ctx, void* stream) {
  if (!ctx) return HMME_ERR_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int flag = 0;
  const int rc = take_flag(ctx, 1, (hipStream_t)stream, &flag);
  if (rc) return rc;
  if (!flag) return HMME_OK;
  return fail(ctx, HMME_ERR_RANGE, "an asynchronous plane upload carried a sample outside the range of its plane's bit depth");
}

uint64_t hmme_test_device_address(const hmme_ctx* ctx, const hmme_plane* pl) {
  if (pl) return (uint64_t)(uintptr_t)pl->origin();
  return ctx ? (uint64_t)(uintptr_t)(ctx->d_call() + kCallCtu) : 0;
}

#ifdef ME_SEARCH_T_TIMELINE   // timing-only builds (tools/search16_timeline.py): the per-workgroup stamps me_search16_kernel left
int hmme_test_timeline16(void* out, size_t bytes) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(hmme::g_timeline16), bytes < sizeof(hmme::g_timeline16) ? bytes : sizeof(hmme::g_timeline16)) == hipSuccess ? HMME_OK : HMME_ERR_DEVICE;
}
#endif
int hmme_test_frac_deal(int k, int n_pairs, int width, int height) {
  if (n_pairs < 1 || width < 8 || height < 8 || width > 16384 || height > 16384) return -1;
  const int n_ctu = hmme_num_ctus(width, height);
  if (n_ctu > 0xffff || k < 0 || k >= n_pairs * n_ctu) return -1;
  const hmme::FracPrep prep = {nullptr, (uint32_t)n_ctu << 16, (uint32_t)width | (uint32_t)height << 16, 0};
  return hmme::me_frac_deal(k, n_pairs * n_ctu, prep);
}

int hmme_test_picture_job(int job, int ctu_first, int ctu_count, int pic_w, int pic_h, int sr, const int16_t* pred_q, const int16_t* center_q, int16_t* out) {
  if (!out || job < 0 || pic_w < 8 || pic_h < 8 || pic_w > 16384 || pic_h > 16384 || sr < 1 || sr > 128) return HMME_ERR_ARG;
  if (ctu_first < 0 || ctu_count < 1 || ctu_first + ctu_count > hmme_num_ctus(pic_w, pic_h)) return HMME_ERR_ARG;
  const MeJob j = hmme::me_picture_job(job, pred_q, center_q, ctu_first, ctu_count, pic_w, pic_h, sr);
  std::memcpy(out, &j, sizeof j);
  return HMME_OK;
}

int hmme_test_stage_layout(const size_t* bytes, int n, size_t* offsets, size_t* total) {
  if (!bytes || !offsets || !total || n < 0) return -1;
  *total = stage_layout(bytes, n, offsets);
  return (int)kStageAlign;
}

int hmme_abi_version(void) { return HMME_ABI_VERSION; }
#ifndef HMME_BUILD_ID
#define HMME_BUILD_ID "unknown"
#endif
const char* hmme_build_id(void) { return HMME_BUILD_ID; }

int hmme_host_register(hmme_ctx* ctx, void* buffer, size_t bytes) {
  if (!ctx) return HMME_ERR_ARG;
  if (!buffer || !bytes) return fail(ctx, HMME_ERR_ARG, "hmme_host_register: null buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipHostRegister(buffer, bytes, hipHostRegisterDefault));
  return HMME_OK;
}

int hmme_host_unregister(hmme_ctx* ctx, void* buffer) {
  if (!ctx) return HMME_ERR_ARG;
  if (!buffer) return fail(ctx, HMME_ERR_ARG, "hmme_host_unregister: null buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipHostUnregister(buffer));
  return HMME_OK;
}

int hmme_plane_set_device_u8(hmme_plane* pl, const void* d_src, int src_pitch, void* stream) {
  if (!pl) return HMME_ERR_ARG;
  if (!d_src || src_pitch < pl->width) return fail(pl->ctx, HMME_ERR_ARG, "hmme_plane_set_device_u8: bad source");
  HIP_TRY(pl->ctx, hipSetDevice(pl->ctx->device));
  if (pl->bps == 1) return plane_fill<uint8_t, uint8_t>(pl, (const uint8_t*)d_src, src_pitch, (hipStream_t)stream, false);
  return plane_fill<uint8_t, uint16_t>(pl, (const uint8_t*)d_src, src_pitch, (hipStream_t)stream, false);
}

// ---- frame search --------------------------------------------------------------------------------------------
// How the (CTU, reference) searches of one launch are dealt to workgroups.  The chip holds ctx->wg_slots search workgroups at a time
// and a launch runs in rounds of that many: 2 040 CTU searches are 3.98 rounds of 512, but 570 (1920 x 1200) are 1.11 -- the second
// round would keep 58 slots busy and cost as much as the first (measured before this plan existed: 2 340 GSAD/s against 3 339 at
// 2160p).  So the jobs beyond the last full round ("tail", from job tail_first on) are dealt in finer pieces:
//   8-bit:  a launch without a tail runs whole jobs (me_search_kernel<FEN, 0>).  With one, ONE launch of me_search_kernel<FEN, 2>: jobs
//           [0, tail_first) whole, one workgroup each and first in the grid; the tail's tasks -- all its jobs' lane-iterations as ONE list --
//           cut into tail_wgs equal segments, one per workgroup (a segment may end one job and begin the next); everything merged
//           through the 64-bit atomicMin table and decoded by me_finalize16_kernel.  Until round 6 every tail job was cut into the same
//           number of pieces: 240 jobs (720p) in 2 pieces each filled 480 of 512 slots with 34 or 33 lane-iterations -- 9 for the
//           slowest wave where 7.85 would do -- and the clipped windows of edge CTUs made shorter pieces still;
//   16-bit: one launch; jobs [0, tail_first) are cut into n_strips strips, tail jobs into tail_parts (>= n_strips).
// A launch of fewer jobs than slots is all tail (the small-picture split mode of round 1).  8-bit windows beyond 129 x 129 (four tiles
// per job through the split kernel) are not re-planned.
enum class SearchMode {
  kWhole8,             // me_search_kernel<FEN, 0>: a workgroup per job, no tail plan
  kTiles8,             // 8-bit windows beyond 129 x 129: four tile searches per job through me_search_kernel<FEN, 1>
  kSegments8,          // head jobs whole and the tail's segments in ONE launch of me_search_kernel<FEN, 2>
  kHeadThenSegments8,  // the head's whole jobs (<FEN, 0>), then the tail's segments (<FEN, 2>): HMME_TAIL_LAUNCHES=2, short tails
  kStrips16            // me_search16_kernel: planes of more than 8 bits, or the u16 copies of a weighted search
};
struct FramePlan {
  SearchMode mode = SearchMode::kWhole8;
  int jobs = 0;
  int n_strips = 1, pdw = 0, strip_rows = 0;   // 16-bit: strips of a head job, the LDS window pitch, most candidate rows of a strip
  int tail_first = 0;      // == jobs: no tail
  int tail_parts = 1;      // 16-bit: strips of a tail job
  int tail_wgs = 0;        // 8-bit: workgroups (= segments) of the tail
  int n_wg16 = 0;          // 16-bit: workgroups of the launch
  size_t table_bytes = 0, table_grow = 0;   // the job table in the context's kJobs, and what a table that has to grow grows to (kMaxRefs references of this picture size)
  size_t tail_jobs_off = 0;   // kHeadThenSegments8: where the tail's segment table (me_seg_table_*) starts in it; the other tables start at its first byte
  bool first_strip = false;   // the launch decodes through kFirstStrip (me_finalize16_kernel): every mode but kWhole8
};

// pieces per tail job that finish `tail` jobs soonest: rounds of `slots` workgroups, each as long as its piece of a whole job
// (cost[k], in any unit) -- ties go to fewer pieces
static int plan_tail(int tail, int slots, int k_min, int k_max, const std::function<double(int)>& cost) {
  int best_k = k_min;
  double best = 1e30;
  for (int k = k_min; k <= k_max; ++k) {
    const double t = (double)(((long)tail * k + slots - 1) / slots) * cost(k);
    if (t < best * 0.999) { best = t; best_k = k; }
  }
  return best_k;
}

// 8-bit launches: workgroups (= segments) for `tail` jobs of full w x w windows beyond the last full round of `slots` workgroups, or 0: the tail
// runs whole in the head's launch.  (pure arithmetic: hmme_test_tail_plan exposes it to the CPU tests)
// the tail's units in `rounds` rounds of `slots` equal segments.  A round costs the lane-iterations of its slowest wave plus what
// every workgroup pays per job it touches -- window load, flush, merge: a quarter iteration fits the sweeps of
// profiles/archive/r02Q_tail_sweeps.txt -- and a segment of u units touches 1 + (u - 1) / units jobs on average.  Full windows are
// assumed (the device counts the clipped ones' units itself: me_prep_segments_kernel).  Never below one unit per workgroup: tiny
// windows get fewer workgroups than slots.
// Segments are whole units of kSegUnit = 4 tasks (one per wave), so a segment of u units costs u lane-iterations.  Against that stands
// the tail run WHOLE in the head's launch -- ceil(nt / 4) lane-iterations per wave for one more round of workgroups, which flow in
// behind the head's without a launch boundary, with the large tasks of whole jobs and without merge table, preset and decode: the
// segment launch is taken only where the model says it wins by 8 % plus half a lane-iteration (1080p's 510 jobs and the 504 left over
// at 2160p stay whole: measured 10 % and 4 % slower as segments, profiles/r06d_tail_segments.txt).
static int plan_tail8(int tail, int slots, int w, int tail_knob) {
  // me_prep_segments_kernel writes prefix[li] for li <= n_jobs from kSegPrepThreads threads: a tail of exactly that many jobs would leave
  // prefix[n_jobs] unwritten.  A 256-CU part (512 slots) has tails of at most 511; a chip with more slots keeps such a tail whole.  (The
  // kernel is left as it is: no chip at hand can run it on a tail of 512.)
  if (tail <= 0 || tail >= hmme::kSegPrepThreads) return 0;
  const int nt = hmme::me_num_tasks(w, w), units = (nt + hmme::kSegUnit - 1) / hmme::kSegUnit;
  const long total = (long)tail * units;
  int best_wgs = 0;
  double best = (double)units + 0.25;   // the tail as whole jobs
  for (int rounds = 1; rounds <= 4; ++rounds) {
    const long wgs = std::max<long>(1, std::min<long>((long)rounds * slots, total));
    const double per_wg = (double)total / wgs;
    const double t = 1.08 * rounds * (std::ceil(per_wg) + 0.25 * (1.0 + (per_wg - 1.0) / units)) + 0.5;
    if (t < best * 0.999) { best = t; best_wgs = (int)wgs; }
    if (wgs < (long)rounds * slots) break;
  }
  if (tail_knob > 1) best_wgs = (int)std::max<long>(1, std::min<long>((long)tail * tail_knob, total));   // A/B: tail_knob workgroups per tail job
  return best_wgs;
}
// head and tail of an 8-bit launch as one segment launch?  One launch lets the tail's segments start on the slots the head's short jobs (clipped
// windows at the picture's edge) leave first, but sends the head's jobs through the merge table and its decode as well: worth it where the tail
// is a good part of the launch (1440p, 408 tail jobs behind 512: +0.4 %; 2560 x 1088, 168: +0.5 %), not for a few jobs behind a full round
// (1200p, 58: -3 %).  profiles/r06n_tail_one_or_two_launches.txt
static bool tail_one_launch(int head, int n_tail, int launches_knob) { return launches_knob == 1 || (launches_knob != 2 && 3 * n_tail >= head); }

// How `jobs` = CTUs x n_refs searches at `search_range` are launched on a chip of `slots` workgroup slots, and the size of their job
// table.  wide: the 16-bit kernel runs them.  Pure arithmetic: no context, no device (hmme_test_tail_plan shows it to the CPU tests).
static FramePlan plan_search(int jobs, int n_refs, int slots, int search_range, bool wide, const Knobs& knobs) {
  FramePlan pl;
  const int w = 2 * search_range + 1, tail = jobs % slots;
  pl.jobs = pl.tail_first = jobs;
  if (wide) {   // strips of equal height for the full window (me_strip_rows16); clipped windows choose their own within n_strips
    pl.mode = SearchMode::kStrips16;
    pl.pdw = pick_pdw16(w);
    const int rmax = pl.strip_rows = rows_max16(pl.pdw), n_min = strips_for(pl.pdw, w);
    const int h = hmme::me_strip_rows16(w, w, rmax, n_min + 4);   // up to four strips more than LDS alone needs
    pl.n_strips = (w + h - 1) / h;
    // the workgroups beyond the last full round: head jobs give (jobs - tail) * n_strips of them, which need not fill whole rounds
    // either -- the tail is planned on what is left of the last head round
    const int lanes = (((w + 1) >> 1) + 2) / 3;
    auto strip_cost = [&](int k) {   // rounds of one strip of a job cut into k, plus half a round for its two window loads
      const int hk = (w + k - 1) / k;
      return 2.0 * ((((hk * lanes + 63) >> 6) + 3) >> 2) + 1.0;
    };
    if (tail && knobs.tail_parts != 1) {
      const int k_max = std::min(w / 4, 64);
      int k = knobs.tail_parts > 1 ? std::min(knobs.tail_parts, k_max) : plan_tail(tail, slots, pl.n_strips, k_max, strip_cost);
      if (k < pl.n_strips) k = pl.n_strips;
      if (k > pl.n_strips) { pl.tail_first = jobs - tail; pl.tail_parts = k; }
    }
    pl.n_wg16 = pl.tail_first * pl.n_strips + (jobs - pl.tail_first) * pl.tail_parts;
    pl.table_bytes = sizeof(MeJob16) * (size_t)pl.n_wg16;
  } else if (search_range > 64) {   // window beyond 129 x 129: four tile searches per CTU, merged like split tasks
    pl.mode = SearchMode::kTiles8;
    pl.table_bytes = sizeof(MeJob16) * (size_t)jobs * 4;
  } else {
    const int wgs = tail && knobs.tail_parts != 1 ? plan_tail8(tail, slots, w, knobs.tail_parts) : 0;
    if (wgs > 0) { pl.tail_first = jobs - tail; pl.tail_wgs = wgs; }
    const int head = pl.tail_first, n_tail = jobs - head;
    if (!n_tail) {
      pl.table_bytes = sizeof(MeJob) * (size_t)head;
    } else if (tail_one_launch(head, n_tail, knobs.tail_launches)) {
      pl.mode = SearchMode::kSegments8;
      pl.table_bytes = hmme::me_seg_table_bytes(head + wgs, jobs);
    } else {
      pl.mode = SearchMode::kHeadThenSegments8;
      pl.tail_jobs_off = (sizeof(MeJob) * (size_t)head + 255) & ~(size_t)255;
      pl.table_bytes = pl.tail_jobs_off + hmme::me_seg_table_bytes(wgs, n_tail);
    }
  }
  pl.first_strip = pl.mode != SearchMode::kWhole8;
  const size_t per_ref = n_refs > 0 ? (pl.table_bytes + n_refs - 1) / n_refs : pl.table_bytes;
  pl.table_grow = per_ref * hmme::kMaxRefs + 4096;
  return pl;
}
// the plan of a launch of the context: force16 = a weighted search of 8-bit planes (its u16 copies)
static FramePlan plan_launch(const hmme_ctx* ctx, const hmme_frame_params* fp, int count, int n_refs, bool force16 = false) {
  return plan_search(count * n_refs, n_refs, ctx->wg_slots, fp->search_range, fp->bit_depth > 8 || force16, knobs());
}

int hmme_test_tail_plan(int width, int height, int search_range, int n_pairs, int slots, int* out) {
  if (!out || width < 8 || height < 8 || width > 16384 || height > 16384 || search_range < 1 || search_range > 64 || n_pairs < 1 || slots < 1) return HMME_ERR_ARG;
  const FramePlan pl = plan_search(hmme_num_ctus(width, height) * n_pairs, n_pairs, slots, search_range, false, Knobs{});
  out[0] = pl.jobs; out[1] = pl.tail_first; out[2] = pl.tail_wgs; out[3] = pl.mode == SearchMode::kSegments8 ? 1 : 0;
  return HMME_OK;
}

int hmme_test_pk_gate(uint32_t lambda_q16) { return hmme::me_pk_gate(lambda_q16) ? 1 : 0; }
int hmme_test_pk_body(uint32_t lambda_q16, int fen) { return hmme::me_pk_body(lambda_q16, fen ? 1 : 0); }
int hmme_test_pk_task_marker_free(int wx, int wy, int k, int it0, int n_it) { return hmme::me_task_marker_free(wx, wy, k, it0, n_it) ? 1 : 0; }
int hmme_test_pk_task_full(int wx, int wy, int k, int it0, int n_it) { return hmme::me_task_full(wx, wy, k, it0, n_it) ? 1 : 0; }
int hmme_test_task_carry_fits(int wx, int wy, int k, int it0, int n_it) { return hmme::me_task_carry_fits(wx, wy, k, it0, n_it) ? 1 : 0; }
int hmme_test_carry_index(int k, int row, int group) {
  if (k < 2 || k > 5 || row < 0 || group < 0 || group >= 1 << (k - 2)) return -1;
  return (int)hmme::me_carry_index(k, row, group);
}
int hmme_test_carry_position(int k, int index, int* out) {
  if (k < 2 || k > 5 || index < 0 || index >= 1 << hmme::kIdxBits || !out) return -1;
  hmme::me_carry_position(k, (uint32_t)index, out[0], out[1]);
  return 0;
}

// writes the device job table of plan `pl` -- a picture search over CTUs [first, first + count) against n_refs reference pictures -- on `s`;
// job index = ref * count + ctu.  kWhole8: MeJob[jobs]; kHeadThenSegments8: MeJob[head], then the tail's segment table; kSegments8: one
// segment table; kTiles8 / kStrips16: MeJob16[workgroups].  A table without predictors or centres that the launch before left is kept.
// d_center_q (16-bit tables only; null = the predictor): the windows' centres of a bi-prediction pass, laid out like d_pred_q
static int prep_jobs(hmme_ctx* ctx, const hmme_plane* cur, const hmme_frame_params* fp, const void* d_pred_q, int first, int count,
                     int n_refs, hipStream_t s, const FramePlan& pl, const void* d_center_q = nullptr) {
  const int jobs = pl.jobs, head = pl.tail_first, n_tail = jobs - head, w = cur->width, h = cur->height, sr = fp->search_range;
  bool moved;
  int rc = ensure(ctx, ctx->buf[kJobs], pl.table_bytes, pl.table_grow, &moved);
  if (moved) ctx->jobs_tag.valid = false;   // reallocated: whatever the table was, it is gone
  if (rc) return rc;
  if (pl.first_strip) {
    rc = ensure(ctx, ctx->buf[kFirstStrip], sizeof(int) * (size_t)jobs, sizeof(int) * (size_t)(jobs / (n_refs > 0 ? n_refs : 1) + 1) * hmme::kMaxRefs, &moved);
    if (moved) ctx->jobs_tag.valid = false;
    if (rc) return rc;
  }
  void* const d_jobs = ctx->buf[kJobs].p;
  int* const d_first_strip = ctx->buf[kFirstStrip].as<int>();
  hmme_ctx::TableTag tag;
  tag.valid = !d_pred_q && !d_center_q;
  tag.w = w; tag.h = h; tag.sr = sr; tag.first = first; tag.count = count; tag.pairs = n_refs;
  tag.bit_depth = fp->bit_depth | (pl.mode == SearchMode::kStrips16 && fp->bit_depth == 8 ? 0x100 : 0);   // 0x100: the 16-bit table of 8-bit planes (weighted search)
  tag.buf = d_jobs; tag.buf2 = pl.first_strip ? d_first_strip : nullptr; tag.stream = (void*)s;
  if (tag.same(ctx->jobs_tag)) return HMME_OK;   // the table of the launch before is this launch's table
  ctx->jobs_tag.valid = false;
  const dim3 block(256);
  const auto grid = [](int n) { return dim3((n + 255) / 256); };
  const int16_t* pred = (const int16_t*)d_pred_q;
  switch (pl.mode) {
    case SearchMode::kTiles8:
      hipLaunchKernelGGL(hmme::me_prep_jobs_tile_kernel, grid(jobs), block, 0, s, (MeJob16*)d_jobs, d_first_strip, pred, first, count, n_refs, w, h, sr);
      break;
    case SearchMode::kStrips16:
      hipLaunchKernelGGL(hmme::me_prep_jobs16_kernel, grid(jobs), block, 0, s, (MeJob16*)d_jobs, d_first_strip, pred, first, count, n_refs, w, h, sr,
                         pl.n_strips, pl.strip_rows, pl.tail_first, pl.tail_parts, (const int16_t*)d_center_q);
      break;
    case SearchMode::kWhole8:
    case SearchMode::kSegments8:
    case SearchMode::kHeadThenSegments8: {
      // kSegments8: one segment table for the whole launch, the head's jobs its entries / workgroups 0 .. head - 1; else the head's MeJobs, then a table of the tail alone
      const int idx0 = pl.mode == SearchMode::kSegments8 ? head : 0;
      if (head && idx0)
        hipLaunchKernelGGL(hmme::me_prep_whole_segments_kernel, grid(head), block, 0, s, d_jobs, d_first_strip, pred, first, count, n_refs, w, h, sr,
                           head + pl.tail_wgs, head);
      else if (head)
        hipLaunchKernelGGL(hmme::me_prep_jobs_kernel, grid(head), block, 0, s, (MeJob*)d_jobs, pred, first, count, n_refs, w, h, sr, 0, head, 1,
                           (uint32_t*)nullptr, (const int16_t*)nullptr);
      if (n_tail)
        hipLaunchKernelGGL(hmme::me_prep_segments_kernel, dim3(1), dim3(hmme::kSegPrepThreads), 0, s, (void*)((uint8_t*)d_jobs + pl.tail_jobs_off), d_first_strip,
                           pred, first, count, n_refs, w, h, sr, idx0 + pl.tail_wgs, head, n_tail, idx0);
      break;
    }
  }
  HIP_TRY(ctx, hipGetLastError());
  ctx->jobs_tag = tag;
  return HMME_OK;
}

// curs: the CTU-blocked copies of the current pictures (hmme_plane::d_blocks), cur_ctus_x their blocks per block row
static int run_search(hmme_ctx* ctx, const RefSet& curs, int cur_ctus_x, const RefSet& refs, int ref_pitch, const hmme_frame_params* fp, const FramePlan& pl,
                      int16_t* d_mv, uint32_t* d_sad, hipStream_t s) {
  const int head = pl.tail_first, n_tail = pl.jobs - head;
  const bool one_launch = pl.mode == SearchMode::kSegments8;
  const void* const d_jobs = ctx->buf[kJobs].p;
  const int* const d_first_strip = ctx->buf[kFirstStrip].as<int>();
  switch (pl.mode) {
    case SearchMode::kStrips16:
      return launch_search16(ctx, curs, cur_ctus_x, refs, ref_pitch, (const MeJob16*)d_jobs, d_first_strip, pl.jobs, pl.n_wg16,
                             pl.pdw, pl.strip_rows, fp->fen, fp->bit_depth, d_mv, d_sad, s);
    case SearchMode::kTiles8:
      return launch_search8_split(ctx, curs, cur_ctus_x, refs, ref_pitch, (const MeJob16*)d_jobs, d_first_strip, pl.jobs, 4,
                                  fp->fen, d_mv, d_sad, s);
    case SearchMode::kWhole8:
      return launch_search8<0>(ctx, curs, cur_ctus_x, refs, ref_pitch, d_jobs, head, fp->fen, d_mv, d_sad, nullptr, 0, s);
    case SearchMode::kSegments8:
    case SearchMode::kHeadThenSegments8: break;
  }
  unsigned long long* best = nullptr;
  int rc = merge_table(ctx, one_launch ? pl.jobs : n_tail, nullptr, s, &best);   // (preset, if it has to be, before the head runs, not between the two)
  if (rc) return rc;
  if (one_launch)
    return launch_search8_segments(ctx, curs, cur_ctus_x, refs, ref_pitch, d_jobs, d_first_strip, pl.jobs, head + pl.tail_wgs, fp->fen, d_mv, d_sad, s, best);
  rc = launch_search8<0>(ctx, curs, cur_ctus_x, refs, ref_pitch, d_jobs, head, fp->fen, d_mv, d_sad, nullptr, 0, s);
  if (rc) return rc;
  return launch_search8_segments(ctx, curs, cur_ctus_x, refs, ref_pitch, (const uint8_t*)d_jobs + pl.tail_jobs_off, d_first_strip, n_tail, pl.tail_wgs,
                                 fp->fen, d_mv + (size_t)head * 2 * HMME_NUM_CTU_PARTS, d_sad + (size_t)head * HMME_NUM_CTU_PARTS, s, best);
}

// n_pairs (current, reference) picture pairs of one size in one launch: validates, orders the streams, fills the two plane sets
namespace {
struct PairLaunch {
  RefSet curs, refs;
  RefSet cur_blocks;   // the current pictures' CTU-blocked copies: what the search kernels read (the refinement reads the padded planes)
  int first = 0, count = 0;
};
int pairs_begin(hmme_ctx* ctx, const hmme_plane* const* curs, const hmme_plane* const* refs, int n_pairs, const hmme_frame_params* fp,
                hipStream_t s, PairLaunch* pl) {
  if (!curs || !refs || n_pairs < 1 || n_pairs > hmme::kMaxRefs) return fail(ctx, HMME_ERR_ARG, "%d picture pairs outside 1..%d", n_pairs, hmme::kMaxRefs);
  pl->curs = one_ref(nullptr); pl->refs = one_ref(nullptr); pl->cur_blocks = one_ref(nullptr);
  for (int r = 0; r < n_pairs; ++r) {
    int rc = check_frame_args(ctx, curs[r], refs[r], fp, &pl->first, &pl->count);
    if (rc) return rc;
    if (refs[r]->pitch != refs[0]->pitch || curs[r]->pitch != curs[0]->pitch || curs[r]->width != curs[0]->width || curs[r]->height != curs[0]->height)
      return fail(ctx, HMME_ERR_ARG, "the planes of one launch differ in size");
    pl->curs.base[r] = curs[r]->origin();
    pl->cur_blocks.base[r] = curs[r]->d_blocks;
    pl->refs.base[r] = refs[r]->origin();
  }
  if (pl->count == 0) return HMME_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc = scratch_acquire(ctx, s);
  for (int r = 0; r < n_pairs && rc == HMME_OK; ++r) {
    rc = plane_wait(ctx, curs[r], s);
    if (rc == HMME_OK) rc = plane_wait(ctx, refs[r], s);
  }
  return rc;
}
// after the kernels are enqueued (or an enqueue failed): the planes have a reader on `s`, the scratch a user
// others (bi-prediction calls; else null): the planes whose prediction the launch subtracted -- read like a reference
int pairs_end(hmme_ctx* ctx, const hmme_plane* const* curs, const hmme_plane* const* refs, int n_pairs, hipStream_t s, int rc,
              const hmme_plane* const* others = nullptr) {
  for (int r = 0; r < n_pairs; ++r) {
    int r2 = (r == 0 || curs[r] != curs[r - 1]) ? plane_read_chain(ctx, curs[r], s) : HMME_OK;
    if (r2 == HMME_OK) r2 = plane_read_chain(ctx, refs[r], s);
    if (r2 == HMME_OK && others) r2 = plane_read_chain(ctx, others[r], s);
    if (rc == HMME_OK) rc = r2;
  }
  // one event for the whole launch (it was one per plane and one for the scratch: 3 .. 33 packets between two kernels of a stream)
  const int r3 = launch_end(ctx, s);
  if (r3 == HMME_OK)
    for (int r = 0; r < n_pairs; ++r) {
      plane_read_mark(ctx, curs[r], s); plane_read_mark(ctx, refs[r], s);
      if (others) plane_read_mark(ctx, others[r], s);
    }
  return rc ? rc : r3;
}
// pairs_end for a launch whose planes do not come in pairs (the *_bi_refs calls: two plane lists of their own lengths): every plane read
// like a reference, one event for all
int lists_end(hmme_ctx* ctx, const hmme_plane* const* a, int na, const hmme_plane* const* b, int nb, hipStream_t s, int rc) {
  const auto at = [&](int r) { return r < na ? a[r] : b[r - na]; };
  for (int r = 0; r < na + nb; ++r) {
    const int r2 = plane_read_chain(ctx, at(r), s);
    if (rc == HMME_OK) rc = r2;
  }
  const int r3 = launch_end(ctx, s);
  if (r3 == HMME_OK)
    for (int r = 0; r < na + nb; ++r) plane_read_mark(ctx, at(r), s);
  return rc ? rc : r3;
}
}  // namespace

int hmme_search_pairs_device(hmme_ctx* ctx, const hmme_plane* const* curs, const hmme_plane* const* refs, int n_pairs,
                             const hmme_frame_params* fp, const void* d_pred_q, void* d_out_mv, void* d_out_sad, void* stream) {
  if (!ctx) return HMME_ERR_ARG;
  if (!d_out_mv || !d_out_sad) return fail(ctx, HMME_ERR_ARG, "null output buffer");
  hipStream_t s = (hipStream_t)stream;
  PairLaunch pl;
  int rc = pairs_begin(ctx, curs, refs, n_pairs, fp, s, &pl);
  if (rc || pl.count == 0) return rc;
  const FramePlan plan = plan_launch(ctx, fp, pl.count, n_pairs);
  rc = prep_jobs(ctx, curs[0], fp, d_pred_q, pl.first, pl.count, n_pairs, s, plan);
  if (rc == HMME_OK) rc = run_search(ctx, pl.cur_blocks, curs[0]->ctus_x, pl.refs, refs[0]->pitch, fp, plan, (int16_t*)d_out_mv, (uint32_t*)d_out_sad, s);
  return pairs_end(ctx, curs, refs, n_pairs, s, rc);
}

int hmme_search_frame_multi_device(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* const* refs, int n_refs,
                                   const hmme_frame_params* fp, const void* d_pred_q, void* d_out_mv, void* d_out_sad, void* stream) {
  if (!ctx) return HMME_ERR_ARG;
  if (!refs || n_refs < 1 || n_refs > hmme::kMaxRefs) return fail(ctx, HMME_ERR_ARG, "n_refs %d outside 1..%d", n_refs, hmme::kMaxRefs);
  const hmme_plane* curs[hmme::kMaxRefs];
  for (int r = 0; r < n_refs; ++r) curs[r] = cur;
  return hmme_search_pairs_device(ctx, curs, refs, n_refs, fp, d_pred_q, d_out_mv, d_out_sad, stream);
}

int hmme_search_frame_device(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* ref, const hmme_frame_params* fp,
                             const void* d_pred_q, void* d_out_mv, void* d_out_sad, void* stream) {
  return hmme_search_frame_multi_device(ctx, cur, &ref, 1, fp, d_pred_q, d_out_mv, d_out_sad, stream);
}

// The synchronous searches' and refinements' way in, behind the checks of their own: the CTU range, the output pointers (a refinement's
// integer MVs too), then -- unless the range is empty: *count == 0, nothing to do -- their items into `st` behind whatever the caller has
// put there, and st.begin().  Up go the predictors of the whole picture and `n_refs` references (null: none) and a refinement's integer
// MVs; st.end() brings back the *count x n_refs result tables.
struct FrameItems { int pred, imv, mv, cost; };
static int stage_in(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* ref, const hmme_frame_params* fp, int n_refs, const int16_t* pred_q,
                    bool refine, const int16_t* int_mv, int16_t* out_mv, uint32_t* out_cost, int* count, Stage& st, FrameItems* it) {
  int first;
  int rc = check_frame_args(ctx, cur, ref, fp, &first, count);
  if (rc) return rc;
  if (refine ? (!int_mv || !out_mv || !out_cost) : (!out_mv || !out_cost)) return fail(ctx, HMME_ERR_ARG, refine ? "null buffer" : "null output buffer");
  if (*count == 0) return HMME_OK;
  const size_t slots = HMME_NUM_CTU_PARTS * (size_t)*count * n_refs;
  it->pred = st.in(pred_q, sizeof(int16_t) * 2 * hmme_num_ctus(cur->width, cur->height) * n_refs);
  it->imv = st.in(int_mv, sizeof(int16_t) * 2 * slots);
  it->mv = st.out(out_mv, sizeof(int16_t) * 2 * slots, 0, sizeof(int16_t) * 2 * slots);
  it->cost = st.out(out_cost, sizeof(uint32_t) * slots, 0, sizeof(uint32_t) * slots);
  return st.begin();
}

int hmme_search_frame_multi(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* const* refs, int n_refs,
                            const hmme_frame_params* fp, const int16_t* pred_q, int16_t* out_mv, uint32_t* out_sad) {
  if (!ctx) return HMME_ERR_ARG;
  if (!refs || n_refs < 1 || n_refs > hmme::kMaxRefs) return fail(ctx, HMME_ERR_ARG, "n_refs %d outside 1..%d", n_refs, hmme::kMaxRefs);
  int count;
  Stage st(ctx);
  FrameItems it;
  int rc = stage_in(ctx, cur, refs[0], fp, n_refs, pred_q, false, nullptr, out_mv, out_sad, &count, st, &it);
  if (rc || count == 0) return rc;
  rc = hmme_search_frame_multi_device(ctx, cur, refs, n_refs, fp, st.at(it.pred), st.at(it.mv), st.at(it.cost), ctx->stream);
  return rc ? rc : st.end();
}

int hmme_search_frame(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* ref, const hmme_frame_params* fp,
                      const int16_t* pred_q, int16_t* out_mv, uint32_t* out_sad) {
  return hmme_search_frame_multi(ctx, cur, &ref, 1, fp, pred_q, out_mv, out_sad);
}

// ---- fractional-pel refinement -------------------------------------------------------------------------------
namespace {
// cover table of me_frac_kernel: for each of the 64 8x8 positions of the CTU the 18 kind-8 slots (width and height
// multiples of 8: 8x8 Hadamard blocks, xGetHADs) that contain it, then for each of the 256 4x4 positions the 6 other
// slots that contain it; ascending slot ids
int build_frac_cover(hmme_ctx* ctx) {
  if (ctx->buf[kFracCover].p) return HMME_OK;
  std::vector<uint16_t> cover;
  for (int kind8 = 1; kind8 >= 0; --kind8) {
    const int step = kind8 ? 8 : 4, per = kind8 ? hmme::kFracCover8 : hmme::kFracCover4;
    for (int py = 0; py < 64; py += step)
      for (int px = 0; px < 64; px += step) {
        int n = 0;
        for (int slot = 0; slot < HMME_NUM_CTU_PARTS; ++slot) {
          int x, y, w, h;
          hmme_slot_rect(slot, &x, &y, &w, &h);
          if (((w % 8 == 0) && (h % 8 == 0)) != (kind8 == 1)) continue;
          if (px >= x && px < x + w && py >= y && py < y + h) { cover.push_back((uint16_t)slot); ++n; }
        }
        if (n != per) return fail(ctx, HMME_ERR_DEVICE, "internal: %d slots cover a %dx%d position, expected %d", n, step, step, per);
      }
  }
  const int rc = ensure(ctx, ctx->buf[kFracCover], sizeof(uint16_t) * cover.size());
  if (rc) return rc;
  HIP_TRY(ctx, hipMemcpy(ctx->buf[kFracCover].p, cover.data(), sizeof(uint16_t) * cover.size(), hipMemcpyHostToDevice));
  return HMME_OK;
}

// One refinement launch, whoever asks for it (plain, weighted, bi-prediction): cover table, job table and counter in kFracJobs, the
// table's kernel where the launch reads one, LDS opt-in, me_frac_kernel.
// kReuse: a table without predictors may be the one the launch before left (frac_jobs_tag); kAsNeeded: written where the launch reads
// one; kAlways: written in any case -- the bi-prediction calls, whose table carries the window centres
enum class FracTable { kReuse, kAsNeeded, kAlways };
struct RefineLaunch {
  RefSet curs, refs;   // one entry per pair of THIS launch
  int cur_pitch = 0, ref_pitch = 0;
  FracBuild build;
  hmme::FracWp fw = kNoWp;
  const int16_t* d_pred = nullptr;     // [pairs][CTUs of the picture][2], null = zero predictors
  const int16_t* d_center = nullptr;   // window centres, same layout; null = the predictors
  int pairs = 0, first = 0, count = 0, width = 0, height = 0, search_range = 0, bit_depth = 0;
  const int16_t* d_int_mv = nullptr;   // [pairs * count][593][2]
  int16_t* d_qmv = nullptr;
  uint32_t* d_cost = nullptr;
  FracTable table = FracTable::kAsNeeded;
};
// what every picture-level refinement takes from its arguments; the caller adds the planes, the build and the predictors
void refine_common(RefineLaunch& L, const PairLaunch& pl, const hmme_plane* cur, const hmme_frame_params* fp, int use_hadamard, const void* d_int_mv,
                   void* d_out_qmv, void* d_out_cost) {
  L.build.had = use_hadamard ? 1 : 0;
  L.first = pl.first; L.count = pl.count; L.width = cur->width; L.height = cur->height; L.search_range = fp->search_range; L.bit_depth = fp->bit_depth;
  L.d_int_mv = (const int16_t*)d_int_mv; L.d_qmv = (int16_t*)d_out_qmv; L.d_cost = (uint32_t*)d_out_cost;
}

int launch_refine(hmme_ctx* ctx, const RefineLaunch& L, hipStream_t s) {
  const int jobs = L.count * L.pairs;
  int rc = build_frac_cover(ctx);
  if (rc) return rc;
  // (a scratch that grows, grows to what kMaxRefs pairs of this CTU range need: the shorter and longer runs of one weighted call fit alike)
  bool moved;
  rc = ensure(ctx, ctx->buf[kFracJobs], sizeof(MeJob) * (size_t)jobs + 64,   // + the launch's job counter behind the table
              sizeof(MeJob) * (size_t)L.count * hmme::kMaxRefs + 4096, &moved);
  if (moved || L.table != FracTable::kReuse) ctx->frac_jobs_tag.valid = false;
  if (rc) return rc;
  MeJob* const d_frac_jobs = ctx->buf[kFracJobs].as<MeJob>();
  uint32_t* counter = (uint32_t*)((uint8_t*)d_frac_jobs + ((sizeof(MeJob) * (size_t)jobs + 15) & ~(size_t)15));
  const int grid = frac_grid(ctx, L.build, jobs);
  // one workgroup per job (the default) on the two-wave builds: every workgroup derives its job itself (FracPrep) -- no job table, no
  // launch in front of this one (1080p: 0.095 -> 0.090 ms).  A table is read by the job-walking launch of HMME_FRAC_GRID (its prep
  // kernel is also what resets the job counter: every launch), under the A/B knob HMME_FRAC_JOB_TABLE (the job table and its kernel as
  // before), by CTU ranges FracPrep cannot pack and by launches with window centres (FracPrep derives windows from predictors only)
  const bool walk = grid < jobs;
  const bool packable = L.count <= 0xffff && L.first <= 0xffff;   // FracPrep packs the CTU range into 16 + 16 bits (a 16384 x 16384 picture has 65 536 CTUs)
  const bool need_table = L.table == FracTable::kAlways || walk || knobs().frac_job_table || !packable || L.d_center;
  if (need_table) {
    hmme_ctx::TableTag tag;
    tag.valid = L.table == FracTable::kReuse && !L.d_pred && !L.d_center && !walk;
    tag.w = L.width; tag.h = L.height; tag.bit_depth = L.bit_depth; tag.sr = L.search_range; tag.first = L.first; tag.count = L.count;
    tag.pairs = L.pairs; tag.buf = d_frac_jobs; tag.stream = (void*)s;
    if (!tag.same(ctx->frac_jobs_tag)) {
      ctx->frac_jobs_tag = tag;
      hipLaunchKernelGGL(hmme::me_prep_jobs_kernel, dim3((jobs + 255) / 256), dim3(256), 0, s, d_frac_jobs, L.d_pred, L.first, L.count, L.pairs,
                         L.width, L.height, L.search_range, 0, jobs, 0, counter, L.d_center);
    }
  }
  rc = frac_lds_optin(ctx, L.build);
  if (rc) return rc;
  // prep: the job of a workgroup without a table (a table carries the predictors itself) and the order the jobs are dealt in
  // (me_frac_deal).  A CTU range beyond 16 + 16 bits gets kNoPrep and with it the plain last-first order.  That is the order such a
  // launch had from every caller: its picture has more than 65 535 CTUs, a packed count holds 65 535 at most, so me_frac_deal's test
  // for a whole picture (count == the picture's CTUs) failed on the overflowed fields too.
  const hmme::FracPrep prep = packable ? hmme::FracPrep{need_table ? nullptr : L.d_pred, (uint32_t)L.first | (uint32_t)L.count << 16,
                                                        (uint32_t)L.width | (uint32_t)L.height << 16, L.search_range}
                                       : kNoPrep;
  hipLaunchKernelGGL(frac_kernel(L.build), dim3(grid), dim3(hmme::frac_threads(L.build.bps())), hmme::frac_lds_bytes(L.build.bps()), s, L.curs,
                     L.cur_pitch, L.refs, L.ref_pitch, need_table ? d_frac_jobs : (const MeJob*)nullptr, prep, jobs,
                     walk ? counter : (uint32_t*)nullptr, ctx->buf[kFracCover].as<uint16_t>(), L.d_int_mv, ctx->lambda_q16, L.bit_depth, L.fw, L.d_qmv, L.d_cost);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? HMME_OK : fail(ctx, HMME_ERR_DEVICE, "refinement launch -> %s", hipGetErrorString(e));
}
}  // namespace

int hmme_refine_pairs_device(hmme_ctx* ctx, const hmme_plane* const* curs, const hmme_plane* const* refs, int n_pairs,
                             const hmme_frame_params* fp, const void* d_pred_q, const void* d_int_mv, int use_hadamard,
                             void* d_out_qmv, void* d_out_cost, void* stream) {
  if (!ctx) return HMME_ERR_ARG;
  if (!d_int_mv || !d_out_qmv || !d_out_cost) return fail(ctx, HMME_ERR_ARG, "null buffer");
  hipStream_t s = (hipStream_t)stream;
  PairLaunch pl;
  int rc = pairs_begin(ctx, curs, refs, n_pairs, fp, s, &pl);
  if (rc || pl.count == 0) return rc;
  RefineLaunch L;
  refine_common(L, pl, curs[0], fp, use_hadamard, d_int_mv, d_out_qmv, d_out_cost);
  L.curs = pl.curs; L.refs = pl.refs; L.cur_pitch = curs[0]->pitch; L.ref_pitch = refs[0]->pitch;
  L.build.wide = curs[0]->bps == 2 ? 1 : 0;
  L.d_pred = (const int16_t*)d_pred_q; L.pairs = n_pairs;
  L.table = FracTable::kReuse;
  return pairs_end(ctx, curs, refs, n_pairs, s, launch_refine(ctx, L, s));
}

int hmme_refine_frame_multi_device(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* const* refs, int n_refs,
                                   const hmme_frame_params* fp, const void* d_pred_q, const void* d_int_mv, int use_hadamard,
                                   void* d_out_qmv, void* d_out_cost, void* stream) {
  if (!ctx) return HMME_ERR_ARG;
  if (!refs || n_refs < 1 || n_refs > hmme::kMaxRefs) return fail(ctx, HMME_ERR_ARG, "n_refs %d outside 1..%d", n_refs, hmme::kMaxRefs);
  const hmme_plane* curs[hmme::kMaxRefs];
  for (int r = 0; r < n_refs; ++r) curs[r] = cur;
  return hmme_refine_pairs_device(ctx, curs, refs, n_refs, fp, d_pred_q, d_int_mv, use_hadamard, d_out_qmv, d_out_cost, stream);
}

int hmme_refine_frame(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* ref, const hmme_frame_params* fp, const int16_t* pred_q,
                      const int16_t* int_mv, int use_hadamard, int16_t* out_qmv, uint32_t* out_cost) {
  int count;
  Stage st(ctx);
  FrameItems it;
  int rc = stage_in(ctx, cur, ref, fp, 1, pred_q, true, int_mv, out_qmv, out_cost, &count, st, &it);
  if (rc || count == 0) return rc;
  rc = hmme_refine_frame_multi_device(ctx, cur, &ref, 1, fp, st.at(it.pred), st.at(it.imv), use_hadamard, st.at(it.mv), st.at(it.cost), ctx->stream);
  return rc ? rc : st.end();
}

// ---- explicit weighted prediction on whole pictures -----------------------------------------------------------
// The picture-level siblings of hmme_search_ctu_w / hmme_refine_ctu_w.  A pair's reference plane is weighted ONCE, margins included, into
// a u16 plane of the context's scratch (me_weight_plane_kernel); its current picture's CTU-blocked copy is widened / biased into a u16
// copy where it has to be (8-bit planes, or a weight whose samples go negative); me_search16_kernel<0, PDW> then runs over them through
// the same job tables, strips and tails as a search of u16 planes.  The refinement interpolates the RAW reference (widened to u16 from
// an 8-bit plane) and weights the clipped prediction per sample: me_frac_kernel<HAD, 2, 1>, one launch per run of equal weights.
namespace {
struct WpInfo { int bias = 0; bool identity = false; };
// the nominal range of the block a weighted reference is compared with, in units of maxv = 2^bitDepth - 1
struct BlockRange { int lo, hi; };
constexpr BlockRange kPictureBlock{0, 1};   // samples of a picture: [0, maxv]
constexpr BlockRange kBiOrigin{-1, 2};      // a bi-prediction origin 2 * org - pred: [-maxv, 2 * maxv]

// what the per-CTU plan decides from the samples a call scans, decided from the nominal ranges -- the reference in [0, 2^bitDepth - 1],
// the block in `block` -- by the same rule (weight_range); the two checks on w0 * sample + round are made here alone
int weight_eval(int bit_depth, const hmme_weight* wp, int refine, BlockRange block, WpInfo* info, char* msg, size_t n) {
  msg[0] = 0;
  if (!wp) { snprintf(msg, n, "null weight"); return HMME_ERR_ARG; }
  if (wp->shift < 0 || wp->shift > 15) { snprintf(msg, n, "weighted prediction: shift %d outside 0..15", wp->shift); return HMME_ERR_ARG; }
  if (bit_depth < 8 || bit_depth > 12) { snprintf(msg, n, "bit depth %d outside 8..12", bit_depth); return HMME_ERR_UNSUPPORTED; }
  const bool identity = wp->w0 == (1 << wp->shift) && wp->offset == 0 && wp->round == (wp->shift ? 1 << (wp->shift - 1) : 0);
  const long maxv = (1L << bit_depth) - 1;
  const long p0 = wp->round, p1 = (long)wp->w0 * maxv + wp->round;   // w0 * ref + round at the two ends of the range (monotonic between)
  // HM forms it in an Int and the device in 32 bits: beyond that nothing is defined
  if (std::min(p0, p1) < INT32_MIN || std::max(p0, p1) > INT32_MAX)
    return refuse(msg, n, HMME_ERR_UNSUPPORTED, "weighted prediction: w0 * sample + round reaches %ld..%ld, beyond 32 bits", std::min(p0, p1), std::max(p0, p1));
  WeightRange wr;
  const int rc = weight_range(wp, 0, maxv, block.lo * maxv, block.hi * maxv, bit_depth - 8, refine != 0, &wr, msg, n);
  if (rc) return rc;
  // me_frac_eval*: fma(w0 * 2^-shift, p, round * 2^-shift) is (w0 * p + round) / 2^shift exactly while the numerator stays below 2^24
  // (identity weights never meet it: they run the unweighted kernel).  The per-CTU calls do not make this check (open points)
  if (refine && !identity && std::max(std::labs(p0), std::labs(p1)) >= (1L << 24))
    return refuse(msg, n, HMME_ERR_UNSUPPORTED, "weighted refinement: w0 * sample + round reaches %ld, beyond what fp32 holds exactly", std::max(std::labs(p0), std::labs(p1)));
  if (info) { info->bias = wr.bias; info->identity = identity; }
  return HMME_OK;
}

// every pair's weight before anything is launched; the message names the pair
int check_weights(hmme_ctx* ctx, const char* who, const hmme_frame_params* fp, const hmme_weight* wps, int n_pairs, int refine, WpInfo* info, bool* all_identity) {
  if (!fp) return fail(ctx, HMME_ERR_ARG, "%s: null params", who);
  if (!wps) return fail(ctx, HMME_ERR_ARG, "%s: null weights", who);
  if (n_pairs < 1 || n_pairs > hmme::kMaxRefs) return fail(ctx, HMME_ERR_ARG, "%d picture pairs outside 1..%d", n_pairs, hmme::kMaxRefs);
  *all_identity = true;
  char msg[256];
  for (int r = 0; r < n_pairs; ++r) {
    const int rc = weight_eval(fp->bit_depth, &wps[r], refine, kPictureBlock, &info[r], msg, sizeof msg);
    if (rc) return fail(ctx, rc, "%s: pair %d: %s", who, r, msg);
    *all_identity = *all_identity && info[r].identity;
  }
  return HMME_OK;
}
inline bool same_weight(const hmme_weight& a, const hmme_weight& b) { return a.w0 == b.w0 && a.offset == b.offset && a.shift == b.shift && a.round == b.round; }
// A weighted refinement runs one launch per run of pairs with equal weights: the weight is one kernel argument (FracWp).
// run_end: the end of the run that begins at pair a (wps == null: no explicit weights, all n pairs are one run)
inline int run_end(const hmme_weight* wps, int a, int n) {
  int b = wps ? a + 1 : n;
  while (b < n && same_weight(wps[b], wps[a])) ++b;
  return b;
}

// geometry of the u16 copies of a launch's planes
struct WpGeom {
  int pitch = 0, rows = 0;
  size_t plane_bytes = 0, origin = 0, blk_bytes = 0;
  explicit WpGeom(const hmme_plane* pl) {
    pitch = ((pl->width + 2 * kMarginX) * 2 + 255) & ~255;   // the pitch of a u16 plane of this size (hmme_plane_create_ex)
    rows = pl->rows;
    plane_bytes = (size_t)pitch * (rows + 1);
    origin = (size_t)kMarginY * pitch + (size_t)kMarginX * 2;
    blk_bytes = (size_t)pl->n_ctu * hmme::kBlkBytes16;
  }
};

// rows x cols samples (u8 or u16) -> u16, ((w0 * v + round) >> shift) + offset_bias each
int weight_pass(hmme_ctx* ctx, int src_bps, const uint8_t* src, int src_pitch, uint8_t* dst, int dst_pitch, long cols, int rows,
                int w0, int round, int shift, int offset_bias, hipStream_t s) {
  const long lanes = cols / (src_bps == 1 ? 16 : 8);   // cols is a multiple of 16 (plane pitches are multiples of 256 bytes, a block is 4096 samples)
  const dim3 grid((unsigned)((lanes + 255) / 256), (unsigned)rows);
  if (src_bps == 1)
    hipLaunchKernelGGL(hmme::me_weight_plane_kernel<uint8_t>, grid, dim3(256), 0, s, src, src_pitch, dst, dst_pitch, (int)cols, w0, round, shift, offset_bias);
  else
    hipLaunchKernelGGL(hmme::me_weight_plane_kernel<uint16_t>, grid, dim3(256), 0, s, src, src_pitch, dst, dst_pitch, (int)cols, w0, round, shift, offset_bias);
  HIP_TRY(ctx, hipGetLastError());
  return HMME_OK;
}
// a whole padded plane (margins included) into the u16 plane `dst` of geometry g
int weight_plane(hmme_ctx* ctx, const hmme_plane* pl, const WpGeom& g, uint8_t* dst, int w0, int round, int shift, int offset_bias, hipStream_t s) {
  return weight_pass(ctx, pl->bps, pl->d_data, pl->pitch, dst, g.pitch, g.pitch / 2, g.rows, w0, round, shift, offset_bias, s);
}
// a plane's CTU-blocked copy into u16 blocks, `bias` added
int bias_blocks(hmme_ctx* ctx, const hmme_plane* pl, uint8_t* dst, int bias, hipStream_t s) {
  return weight_pass(ctx, pl->bps, pl->d_blocks, 0, dst, 0, (long)pl->n_ctu * 64 * 64, 1, 1, 0, 0, bias, s);
}

// The u16 copies the pairs of one launch take from one scratch buffer (d_wp[k]): pair r's copy goes into slot r, unless a pair before it
// has made the same copy -- the same plane through the same arithmetic (what weight_pass gets) -- which then serves both.
struct CopyKey { const hmme_plane* pl; int w0, round, shift, offset_bias; };
struct CopyCache {
  uint8_t* scratch; size_t slot_bytes;
  bool blocks;   // copies of the CTU-blocked picture (bias_blocks) rather than of the padded plane (weight_plane: the copy's address is its origin)
  CopyKey key[hmme::kMaxRefs]; const uint8_t* copy[hmme::kMaxRefs];   // per pair: what it asked for and got (null: nothing)
  CopyCache(uint8_t* scratch_, size_t slot_bytes_, bool blocks_) : scratch(scratch_), slot_bytes(slot_bytes_), blocks(blocks_), key{}, copy{} {}
};
int cached_copy(hmme_ctx* ctx, CopyCache& cc, const WpGeom& g, int r, const CopyKey& k, hipStream_t s, const uint8_t** out) {
  int q = 0, rc = HMME_OK;
  const auto same = [&](const CopyKey& o) { return o.pl == k.pl && o.w0 == k.w0 && o.round == k.round && o.shift == k.shift && o.offset_bias == k.offset_bias; };
  while (q < r && !(cc.copy[q] && same(cc.key[q]))) ++q;
  if (q < r) {
    cc.copy[r] = cc.copy[q];
  } else {
    uint8_t* dst = cc.scratch + cc.slot_bytes * r;
    rc = cc.blocks ? bias_blocks(ctx, k.pl, dst, k.offset_bias, s) : weight_plane(ctx, k.pl, g, dst, k.w0, k.round, k.shift, k.offset_bias, s);
    cc.copy[r] = cc.blocks ? dst : dst + g.origin;
  }
  cc.key[r] = k;
  *out = cc.copy[r];
  return rc;
}
}  // namespace

int hmme_weight_check(int bit_depth, const hmme_weight* wp, int refine) {
  char msg[256];
  return weight_eval(bit_depth, wp, refine, kPictureBlock, nullptr, msg, sizeof msg);
}

int hmme_search_pairs_w_device(hmme_ctx* ctx, const hmme_plane* const* curs, const hmme_plane* const* refs, int n_pairs,
                               const hmme_frame_params* fp, const hmme_weight* wps, const void* d_pred_q, void* d_out_mv, void* d_out_sad,
                               void* stream) {
  if (!ctx) return HMME_ERR_ARG;
  WpInfo info[hmme::kMaxRefs];
  bool all_identity = false;
  int rc = check_weights(ctx, "hmme_search_pairs_w_device", fp, wps, n_pairs, 0, info, &all_identity);
  if (rc) return rc;
  if (!d_out_mv || !d_out_sad) return fail(ctx, HMME_ERR_ARG, "null output buffer");
  hmme_frame_params f = *fp;
  f.fen = 0;   // xGetSADw reads every row (TComRdCost.cpp:467-469): FEN is not consulted
  if (all_identity) return hmme_search_pairs_device(ctx, curs, refs, n_pairs, &f, d_pred_q, d_out_mv, d_out_sad, stream);   // the prediction IS the reference
  hipStream_t s = (hipStream_t)stream;
  PairLaunch pl;
  rc = pairs_begin(ctx, curs, refs, n_pairs, &f, s, &pl);
  if (rc || pl.count == 0) return rc;
  const WpGeom g(refs[0]);
  rc = ensure(ctx, ctx->buf[kWp0], g.plane_bytes * n_pairs);
  if (rc == HMME_OK) rc = ensure(ctx, ctx->buf[kWp1], g.blk_bytes * n_pairs);
  RefSet wrefs = one_ref(nullptr), wcurs = one_ref(nullptr);
  CopyCache wref(ctx->wp(0), g.plane_bytes, false), wcur(ctx->wp(1), g.blk_bytes, true);
  for (int r = 0; r < n_pairs && rc == HMME_OK; ++r) {
    const hmme_weight& w = wps[r];
    rc = cached_copy(ctx, wref, g, r, CopyKey{refs[r], w.w0, w.round, w.shift, w.offset + info[r].bias}, s, &wrefs.base[r]);
    if (rc != HMME_OK) break;
    if (curs[r]->bps == 2 && info[r].bias == 0) wcurs.base[r] = curs[r]->d_blocks;   // the plane's own blocks serve
    else rc = cached_copy(ctx, wcur, g, r, CopyKey{curs[r], 1, 0, 0, info[r].bias}, s, &wcurs.base[r]);
  }
  const FramePlan plan = plan_launch(ctx, &f, pl.count, n_pairs, true);
  if (rc == HMME_OK) rc = prep_jobs(ctx, curs[0], &f, d_pred_q, pl.first, pl.count, n_pairs, s, plan);
  if (rc == HMME_OK) rc = run_search(ctx, wcurs, curs[0]->ctus_x, wrefs, g.pitch, &f, plan, (int16_t*)d_out_mv, (uint32_t*)d_out_sad, s);
  return pairs_end(ctx, curs, refs, n_pairs, s, rc);
}

int hmme_search_frame_w(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* ref, const hmme_frame_params* fp, const hmme_weight* wp,
                        const int16_t* pred_q, int16_t* out_mv, uint32_t* out_sad) {
  if (!ctx) return HMME_ERR_ARG;
  WpInfo info;
  bool identity = false;
  int rc = check_weights(ctx, "hmme_search_frame_w", fp, wp, 1, 0, &info, &identity);
  if (rc) return rc;
  int count;
  Stage st(ctx);
  FrameItems it;
  rc = stage_in(ctx, cur, ref, fp, 1, pred_q, false, nullptr, out_mv, out_sad, &count, st, &it);
  if (rc || count == 0) return rc;
  rc = hmme_search_pairs_w_device(ctx, &cur, &ref, 1, fp, wp, st.at(it.pred), st.at(it.mv), st.at(it.cost), ctx->stream);
  return rc ? rc : st.end();
}

int hmme_refine_pairs_w_device(hmme_ctx* ctx, const hmme_plane* const* curs, const hmme_plane* const* refs, int n_pairs,
                               const hmme_frame_params* fp, const hmme_weight* wps, const void* d_pred_q, const void* d_int_mv, int use_hadamard,
                               void* d_out_qmv, void* d_out_cost, void* stream) {
  if (!ctx) return HMME_ERR_ARG;
  WpInfo info[hmme::kMaxRefs];
  bool all_identity = false;
  int rc = check_weights(ctx, "hmme_refine_pairs_w_device", fp, wps, n_pairs, 1, info, &all_identity);
  if (rc) return rc;
  if (!d_int_mv || !d_out_qmv || !d_out_cost) return fail(ctx, HMME_ERR_ARG, "null buffer");
  if (all_identity) return hmme_refine_pairs_device(ctx, curs, refs, n_pairs, fp, d_pred_q, d_int_mv, use_hadamard, d_out_qmv, d_out_cost, stream);
  hipStream_t s = (hipStream_t)stream;
  PairLaunch pl;
  rc = pairs_begin(ctx, curs, refs, n_pairs, fp, s, &pl);
  if (rc || pl.count == 0) return rc;
  const int src_wide = curs[0]->bps == 2 ? 1 : 0, n_ctu = curs[0]->n_ctu;
  const WpGeom g(refs[0]);
  bool need_cur = false;
  for (int r = 0; r < n_pairs; ++r) need_cur = need_cur || (!info[r].identity && (!src_wide || info[r].bias));
  if (!src_wide) rc = ensure(ctx, ctx->buf[kWp2], g.plane_bytes * n_pairs);
  if (rc == HMME_OK && need_cur) rc = ensure(ctx, ctx->buf[kWp3], g.plane_bytes * n_pairs);
  CopyCache raw(ctx->wp(2), g.plane_bytes, false), wcur(ctx->wp(3), g.plane_bytes, false);   // references widened to u16 / current pictures widened and biased
  // one launch per run of pairs with equal weights: the weight is one kernel argument (FracWp)
  for (int a = 0, b; a < n_pairs && rc == HMME_OK; a = b) {
    b = run_end(wps, a, n_pairs);
    const bool ident = info[a].identity;   // the prediction is the reference: the unweighted kernel on the planes themselves
    const int wide = ident ? src_wide : 1;
    RefSet c = one_ref(nullptr), rf = one_ref(nullptr);
    for (int r = a; r < b && rc == HMME_OK; ++r) {
      if (ident) { c.base[r - a] = pl.curs.base[r]; rf.base[r - a] = pl.refs.base[r]; continue; }
      // the RAW reference is interpolated; the current samples carry the bias (FracWp::org_sub takes it off again, with the offset)
      if (src_wide) rf.base[r - a] = pl.refs.base[r];
      else rc = cached_copy(ctx, raw, g, r, CopyKey{refs[r], 1, 0, 0, 0}, s, &rf.base[r - a]);
      if (rc != HMME_OK) break;
      if (src_wide && info[r].bias == 0) c.base[r - a] = pl.curs.base[r];
      else rc = cached_copy(ctx, wcur, g, r, CopyKey{curs[r], 1, 0, 0, info[r].bias}, s, &c.base[r - a]);
    }
    if (rc != HMME_OK) break;
    // the run's own table and counter, where it reads one, in the same buffer as the run before (on one stream: behind its kernel)
    const size_t res0 = (size_t)a * pl.count * HMME_NUM_CTU_PARTS;
    RefineLaunch L;
    refine_common(L, pl, curs[0], fp, use_hadamard, (const int16_t*)d_int_mv + 2 * res0, (int16_t*)d_out_qmv + 2 * res0, (uint32_t*)d_out_cost + res0);
    L.curs = c; L.refs = rf;
    L.cur_pitch = ident ? curs[0]->pitch : g.pitch; L.ref_pitch = ident ? refs[0]->pitch : g.pitch;   // (a u16 plane's own pitch is g.pitch)
    L.build.wide = wide; L.build.wp = ident ? 0 : 1;
    if (!ident) L.fw = frac_wp(&wps[a], info[a].bias);
    L.d_pred = d_pred_q ? (const int16_t*)d_pred_q + (size_t)a * n_ctu * 2 : nullptr; L.pairs = b - a;
    rc = launch_refine(ctx, L, s);
  }
  return pairs_end(ctx, curs, refs, n_pairs, s, rc);
}

int hmme_refine_frame_w(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* ref, const hmme_frame_params* fp, const hmme_weight* wp,
                        const int16_t* pred_q, const int16_t* int_mv, int use_hadamard, int16_t* out_qmv, uint32_t* out_cost) {
  if (!ctx) return HMME_ERR_ARG;
  WpInfo info;
  bool identity = false;
  int rc = check_weights(ctx, "hmme_refine_frame_w", fp, wp, 1, 1, &info, &identity);
  if (rc) return rc;
  int count;
  Stage st(ctx);
  FrameItems it;
  rc = stage_in(ctx, cur, ref, fp, 1, pred_q, true, int_mv, out_qmv, out_cost, &count, st, &it);
  if (rc || count == 0) return rc;
  rc = hmme_refine_pairs_w_device(ctx, &cur, &ref, 1, fp, wp, st.at(it.pred), st.at(it.imv), use_hadamard, st.at(it.mv), st.at(it.cost), ctx->stream);
  return rc ? rc : st.end();
}

// ---- bi-prediction on whole pictures and picture pairs ----------------------------------------------------------
// The picture-level form of the bBi pass of the per-CTU calls.  For every pair the other list's prediction is motion-compensated from a
// motion field and folded into the current picture's CTU blocks as 2 * cur - pred + bias (me_predict_kernel<SrcT, 1>, one launch per pair,
// bias = 2^bitDepth - 1: the origin lies in [-maxv, 2 * maxv]); the reference gets a u16 copy with the same bias (me_weight_plane_kernel at
// weight 1, once per distinct plane) and me_search16_kernel runs over the two through the job tables, strips and tails of any u16 search --
// the window centred on d_center_q where the caller gives one (me_prep_jobs16_kernel).  The refinement writes the origin into a padded u16
// plane instead (the refinement kernel reads its current block by pitch) and runs me_frac_kernel<HAD, 2, 1> with the identity weight and
// org_sub = bias on the RAW reference: the plane itself above 8 bits, a widened copy at 8 (DESIGN.md 7 gives the reason for this choice).
// With explicit weights (the *_w calls) the searched list's weight prices the candidates (xGetSADw / xGetHADsw: the copy of the reference is
// weighted, the refinement runs one launch per run of equal searched weights) and the other list's shapes the prediction the origin is built
// from (addWeightUni).  A launch whose weights are all the identity IS the unweighted call with FEN off.
// Two forms share the bodies below (BiLaunch, bi_search, bi_refine).  The PAIRS form (hmme_*_pairs_bi*, hmme_*_frame_bi, _bi_w) searches n
// picture pairs, each against the prediction from its own plane and motion field of the other list; the LISTS form (hmme_*_frame_bi_refs*; the
// rule: include/hmme.h) searches one picture against all references of a list, the other list's prediction coming from a reference per block,
// others[d_other_ref[block]].  They differ in four things:
//   origins  one per pair, from others[r] with the field at field * r -- or ONE for the launch, as the multi-reference uni launch hands one
//            current picture to its pairs (me_predict_kernel<T, 1, 0 | 2, 1>, one launch per call); the biased / raw copies stay per reference
//   bias     the pair's own -- or ONE for all references, the largest of the searched weights' own (weight_eval); every weighted copy then
//            carries offset_r + bias
//   weights  of the other list: one MePredWp<1> per origin launch (pw) -- or all of them in the one launch (pr with prw)
//   tail     the planes come in pairs (pairs_end) -- or in two lists of their own lengths (lists_end)
namespace {
// what the kernels hold, from the nominal sample range: origin in [-maxv, 2 maxv], reference in [0, maxv]
int bipred_eval(int bit_depth, int refine, char* msg, size_t n) {
  msg[0] = 0;
  if (bit_depth < 8 || bit_depth > 12) { snprintf(msg, n, "bit depth %d outside 8..12", bit_depth); return HMME_ERR_ARG; }
  const long maxv = (1L << bit_depth) - 1;
  if (3 * maxv > 65535) { snprintf(msg, n, "bi-prediction origins of %d-bit samples span more than 16 bits", bit_depth); return HMME_ERR_UNSUPPORTED; }
  const long span = 2 * maxv;   // largest |origin - reference sample|
  if (((4096 * span) >> (bit_depth - 8)) + 65535 >= (long)hmme::kInvCost16) {
    snprintf(msg, n, "bi-prediction SADs of a %d-bit block could reach %ld: beyond the cost field", bit_depth, 4096 * span);
    return HMME_ERR_UNSUPPORTED;
  }
  if (refine && 4096 * span >= (1L << 24)) {
    snprintf(msg, n, "bi-prediction refinement at %d bits: sample differences up to %ld exceed what the Hadamard sums hold exactly", bit_depth, span);
    return HMME_ERR_UNSUPPORTED;
  }
  return HMME_OK;
}

int bi_check(hmme_ctx* ctx, const char* who, const hmme_frame_params* fp, int refine) {
  if (!fp) return fail(ctx, HMME_ERR_ARG, "%s: null params", who);
  char msg[256];
  const int rc = bipred_eval(fp->bit_depth, refine, msg, sizeof msg);
  return rc ? fail(ctx, rc, "%s: %s", who, msg) : HMME_OK;
}

// the argument checks of a bi-prediction launch that pairs_begin does not make
int bi_args(hmme_ctx* ctx, const char* who, const hmme_plane* const* curs, const hmme_plane* const* refs, const hmme_plane* const* others, int n_pairs,
            const hmme_frame_params* fp, const void* d_other_mv, int mv_per_ctu, bool four = false) {
  if (!curs || !refs || !others || n_pairs < 1 || n_pairs > hmme::kMaxRefs) return fail(ctx, HMME_ERR_ARG, "%s: %d picture pairs outside 1..%d (or a null plane list)", who, n_pairs, hmme::kMaxRefs);
  // the *_bi4 entries (four) are the 256 layout and nothing else; every other entry takes 1 or 64
  if (!d_other_mv || (four ? mv_per_ctu != 256 : (mv_per_ctu != 1 && mv_per_ctu != 64)))
    return fail(ctx, HMME_ERR_ARG, "%s: null motion field, or %d MVs per CTU (%s)", who, mv_per_ctu, four ? "256" : "1 or 64");
  for (int r = 0; r < n_pairs; ++r) {
    if (!curs[r] || !refs[r] || !others[r]) return fail(ctx, HMME_ERR_ARG, "%s: null plane", who);
    if (others[r]->ctx != ctx) return fail(ctx, HMME_ERR_ARG, "plane belongs to another context (planes are used with the context that created them)");
    if (others[r]->width != curs[r]->width || others[r]->height != curs[r]->height) return fail(ctx, HMME_ERR_ARG, "%s: pair %d: the other list's plane differs in size", who, r);
    if (others[r]->bit_depth != fp->bit_depth) return fail(ctx, HMME_ERR_ARG, "%s: pair %d: the other list's plane holds %d-bit samples, the call asks for %d", who, r, others[r]->bit_depth, fp->bit_depth);
  }
  return HMME_OK;
}

// The weights of a bi launch as the kernels take them.  Per searched pair r: the bias its origin and weighted reference carry and whether
// its weight is the identity, as weight_eval reads the word (round included); in the lists form every bias is the common maximum.  Per pair
// or plane k of the other list: its weight as addWeightUni forms it, and whether it is the identity (the prediction family's meaning).
// Without explicit weights: bias maxv, all identities.
struct BiWp {
  int bias[hmme::kMaxRefs] = {};
  bool identity[hmme::kMaxRefs] = {};
  hmme::MePredWp<2> other = {};
  bool other_identity[hmme::kMaxRefs] = {};
  bool others_identity = true;   // every other weight: the lists form's origin is the unweighted one
  bool all_identity = true;      // every weight of both lists: the call IS the unweighted one with fen = 0
  static BiWp unweighted(int bit_depth) {
    BiWp bw;
    for (int r = 0; r < hmme::kMaxRefs; ++r) { bw.bias[r] = (1 << bit_depth) - 1; bw.identity[r] = bw.other_identity[r] = true; }
    return bw;
  }
};

// What is an argument error in every weight of the bi family, before any range is looked at: bit depth, null, shift.  (weight_eval, the
// *_w family's check, answers HMME_ERR_UNSUPPORTED to a bit depth outside 8..12 and keeps doing so; the bi family follows hmme_bipred_check,
// which answers HMME_ERR_ARG, so the depth is tested here first and weight_eval never sees a bad one.)
int bi_weight_args(int bit_depth, const hmme_weight* wp, const char* which, char* msg, size_t n) {
  msg[0] = 0;
  if (bit_depth < 8 || bit_depth > 12) { snprintf(msg, n, "bit depth %d outside 8..12", bit_depth); return HMME_ERR_ARG; }
  if (!wp) { snprintf(msg, n, "null weight of the %s list", which); return HMME_ERR_ARG; }
  if (wp->shift < 0 || wp->shift > 15) { snprintf(msg, n, "weighted prediction of the %s list: shift %d outside 0..15", which, wp->shift); return HMME_ERR_ARG; }
  return HMME_OK;
}

// the other list's weight (TComWeightPrediction.cpp:133-180): ClipBD(((w0 * (P + 8192) + round') >> shift') + offset) with
// shift' = shift + headRoom and round' = 1 << (shift' - 1); wp->round is not used.  P is a Pel, so P + 8192 lies within [-24 576, 40 959]
// (what the reference's filters reach on the worst-case, tap-sign content: luma -25 085 .. 25 079, chroma -14 112 .. 14 106, tests/golden/ref_blocks.npz).
int other_weight_eval(int bit_depth, const hmme_weight* wp, bool* identity, hmme::MePredWp<1>* pw, char* msg, size_t n, const char* which = "other") {
  const int rc = bi_weight_args(bit_depth, wp, which, msg, n);
  if (rc) return rc;
  const int sh = wp->shift + std::max(2, 14 - bit_depth);
  const long rnd = 1L << (sh - 1);
  if (std::labs((long)wp->w0) * 40960 + rnd > INT32_MAX) {
    snprintf(msg, n, "weighted prediction of the %s list: |w0| * 40960 + round' reaches %ld, beyond 32 bits", which, std::labs((long)wp->w0) * 40960 + rnd);
    return HMME_ERR_UNSUPPORTED;
  }
  if (identity) *identity = wp->w0 == (1 << wp->shift) && wp->offset == 0;
  if (pw) *pw = hmme::MePredWp<1>{wp->w0, (int)rnd, sh, wp->offset};
  return HMME_OK;
}

// the range checks of one weight of a bi launch, and what the kernels take from it into the summary (bw null: the check alone): searched
// weight r against a bi-prediction origin, other weight k
int bi_searched_eval(int bit_depth, const hmme_weight* wp, int refine, BiWp* bw, int r, char* msg, size_t n) {
  WpInfo info;
  const int rc = weight_eval(bit_depth, wp, refine, kBiOrigin, &info, msg, n);
  if (rc == HMME_OK && bw) { bw->bias[r] = info.bias; bw->identity[r] = info.identity; bw->all_identity = bw->all_identity && info.identity; }
  return rc;
}
int bi_other_eval(int bit_depth, const hmme_weight* wp, BiWp* bw, int k, char* msg, size_t n) {
  bool id = true;
  hmme::MePredWp<1> pw;
  const int rc = other_weight_eval(bit_depth, wp, &id, &pw, msg, n);
  if (rc == HMME_OK && bw) {
    bw->other.ref[k] = pw; bw->other_identity[k] = id;
    bw->others_identity = bw->others_identity && id; bw->all_identity = bw->all_identity && id;
  }
  return rc;
}

// both weights of pair r: the argument errors of both first, then the searched list's ranges against a bi-prediction origin, then the
// other list's
int bipred_weight_eval(int bit_depth, const hmme_weight* wp, const hmme_weight* other_wp, int refine, BiWp* bw, int r, char* msg, size_t n) {
  int rc = bi_weight_args(bit_depth, wp, "searched", msg, n);
  if (rc == HMME_OK) rc = bi_weight_args(bit_depth, other_wp, "other", msg, n);
  if (rc == HMME_OK) rc = bi_searched_eval(bit_depth, wp, refine, bw, r, msg, n);
  if (rc == HMME_OK) rc = bi_other_eval(bit_depth, other_wp, bw, r, msg, n);
  return rc;
}

// The two weights of a picture whose blocks are L0, L1 or bi (hmme_predict_bi_w_device; the rule: include/hmme.h): the argument errors of
// both first, then each weight alone -- uni-directional blocks go through addWeightUni with it --, then the pair in addWeightBi
// (TComWeightPrediction.cpp:46-49, :67-129, getWpScaling :230-247): shift' = shift + 1 + headRoom, round' = 1 << (shift' - 1), the two
// offsets summed and multiplied by 2^(shift' - 1).  P + 8192 lies within [-24 576, 40 959] for each list.
struct PredBiWp {
  bool identity = true;   // both weights: the picture is hmme_predict_bi_device's
  hmme::MePredBiWp<1> k{};
};
int predict_bi_weight_eval(int bit_depth, const hmme_weight* wp0, const hmme_weight* wp1, PredBiWp* out, char* msg, size_t n) {
  int rc = bi_weight_args(bit_depth, wp0, "L0", msg, n);
  if (rc == HMME_OK) rc = bi_weight_args(bit_depth, wp1, "L1", msg, n);
  if (rc) return rc;
  if (wp0->shift != wp1->shift) {
    snprintf(msg, n, "weighted bi-prediction: shifts %d and %d differ (luma has one log2WeightDenom per slice)", wp0->shift, wp1->shift);
    return HMME_ERR_ARG;
  }
  bool id[2];
  hmme::MePredWp<1> uni[2];
  rc = other_weight_eval(bit_depth, wp0, &id[0], &uni[0], msg, n, "L0");
  if (rc == HMME_OK) rc = other_weight_eval(bit_depth, wp1, &id[1], &uni[1], msg, n, "L1");
  if (rc) return rc;
  const int sh = wp0->shift + 1 + std::max(2, 14 - bit_depth);
  const int64_t rnd = (int64_t)1 << (sh - 1), off = (int64_t)wp0->offset + wp1->offset;
  const int64_t reach = (std::llabs((long long)wp0->w0) + std::llabs((long long)wp1->w0)) * 40960 + rnd + std::llabs((long long)off) * rnd;
  if (reach > INT32_MAX) {
    snprintf(msg, n, "weighted bi-prediction: (|w0| + |w1|) * 40960 + round' + |offset0 + offset1| * 2^(shift' - 1) reaches %lld, beyond 32 bits", (long long)reach);
    return HMME_ERR_UNSUPPORTED;
  }
  if (out) {
    out->identity = id[0] && id[1];
    out->k = hmme::MePredBiWp<1>{wp0->w0, wp1->w0, (int)(rnd + off * rnd), sh, {uni[0], uni[1]}};
  }
  return HMME_OK;
}

// every pair's two weights before anything is launched; the message names the pair
int check_bi_weights(hmme_ctx* ctx, const char* who, const hmme_frame_params* fp, const hmme_weight* wps, const hmme_weight* other_wps, int n_pairs, int refine,
                     BiWp* bw) {
  if (!fp) return fail(ctx, HMME_ERR_ARG, "%s: null params", who);
  if (!wps || !other_wps) return fail(ctx, HMME_ERR_ARG, "%s: null weights", who);
  if (n_pairs < 1 || n_pairs > hmme::kMaxRefs) return fail(ctx, HMME_ERR_ARG, "%s: %d picture pairs outside 1..%d", who, n_pairs, hmme::kMaxRefs);
  *bw = BiWp{};
  char msg[256];
  for (int r = 0; r < n_pairs; ++r) {
    const int rc = bipred_weight_eval(fp->bit_depth, &wps[r], &other_wps[r], refine, bw, r, msg, sizeof msg);
    if (rc) return fail(ctx, rc, "%s: pair %d: %s", who, r, msg);
  }
  return HMME_OK;
}

// The one way a predict launch picks its instantiation: f is called with a value of the planes' sample type (bps 1: uint8_t, 2: uint16_t),
// and names its kernel with decltype of it.
extern "C++" {
template <class F>
void with_sample_type(int bps, F&& f) {
  if (bps == 1) f(uint8_t{}); else f(uint16_t{});
}
}  // extern "C++"

// me_predict_kernel for CTUs [first, first + count) of `src` with its motion field (int16 [n_ctu][mv_per_ctu][2], device)
// pw: the weight of a slice with explicit weighted prediction (null: none, and the identity -- WP = 0 computes the same samples)
// pr: a reference picture per block (hmme_predict_refs_device; `src` gives the geometry all planes share), prw: with one weight per
// reference (hmme_predict_refs_w_device; null: none); origin with pr: the origin of the *_bi_refs calls, with prw too: of the *_bi_refs_w calls
int launch_predict(hmme_ctx* ctx, const hmme_plane* src, const int16_t* d_field, int mv_per_ctu, int first, int count, bool origin, const uint8_t* cur_blocks,
                   int bias, uint8_t* dst, long dst_ctu_x, long dst_ctu_y, int dst_pitch, hipStream_t s, const hmme::MePredWp<1>* pw = nullptr,
                   const hmme::MePredRefs<1>* pr = nullptr, const hmme::MePredWp<2>* prw = nullptr) {
  with_sample_type(src->bps, [&](auto sample) {
    using T = decltype(sample);
    const auto go = [&](auto kernel, auto wp, auto refs) {
      hipLaunchKernelGGL(kernel, dim3((unsigned)count), dim3(256), 0, s, src->origin(), src->pitch, d_field, mv_per_ctu, first, src->width, src->height,
                         src->bit_depth, cur_blocks, bias, dst, dst_ctu_x, dst_ctu_y, dst_pitch, wp, refs);
    };
    const hmme::MePredWp<0> no_wp;
    const hmme::MePredRefs<0> no_refs;
    if (origin && pr && prw) go(hmme::me_predict_kernel<T, 1, 2, 1>, *prw, *pr);
    else if (pr && prw) go(hmme::me_predict_kernel<T, 0, 2, 1>, *prw, *pr);
    else if (origin && pr) go(hmme::me_predict_kernel<T, 1, 0, 1>, no_wp, *pr);
    else if (pr) go(hmme::me_predict_kernel<T, 0, 0, 1>, no_wp, *pr);
    else if (origin && pw) go(hmme::me_predict_kernel<T, 1, 1, 0>, *pw, no_refs);
    else if (origin) go(hmme::me_predict_kernel<T, 1, 0, 0>, no_wp, no_refs);
    else if (pw) go(hmme::me_predict_kernel<T, 0, 1, 0>, *pw, no_refs);
    else go(hmme::me_predict_kernel<T, 0, 0, 0>, no_wp, no_refs);
  });
  HIP_TRY(ctx, hipGetLastError());
  return HMME_OK;
}

// me_predict4_kernel for CTUs [first, first + count) of a picture like `src`: one MV and one reference index (d_ref_field null: 0) per 4x4
// block, every plane of `set`; prw: one weight per reference (null: none, and identities); org: the bi-prediction origin of the *_bi4 calls
// instead of the prediction (unweighted), dst / dst_pitch then being the origin's
int launch_predict4(hmme_ctx* ctx, const hmme_plane* src, const hmme::RefSet& set, int n_refs, const int16_t* d_field, const uint8_t* d_ref_field, int first, int count,
                    uint8_t* dst, int dst_pitch, hipStream_t s, const hmme::MePredWp<2>* prw, const hmme::MePred4Origin<1>* org = nullptr) {
  with_sample_type(src->bps, [&](auto sample) {
    using T = decltype(sample);
    const auto go = [&](auto kernel, auto wp, auto origin) {
      hipLaunchKernelGGL(kernel, dim3((unsigned)count), dim3(256), 0, s, set, n_refs, src->pitch, d_field, d_ref_field, first, src->width, src->height, src->bit_depth, dst,
                         dst_pitch, wp, origin);
    };
    const hmme::MePred4Origin<0> none;
    if (org) go(hmme::me_predict4_kernel<T, 0, 1>, hmme::MePredWp<0>{}, *org);
    else if (prw) go(hmme::me_predict4_kernel<T, 2>, *prw, none);
    else go(hmme::me_predict4_kernel<T, 0>, hmme::MePredWp<0>{}, none);
  });
  HIP_TRY(ctx, hipGetLastError());
  return HMME_OK;
}

// me_predict_bi_kernel (mv_per_ctu 1 | 64) or me_predict_bi4_kernel (256: unweighted) for CTUs [first, first + count) of a picture like `src`
// with a direction per block (d_dirs) and list-major MVs: list 0 from ref0, list 1 from ref1.  pw: the picture's weights (null: none, and
// identities); pr: a reference per block and list instead of ref0 / ref1 (hmme_predict_bi_refs_device), prw: with one weight per reference
int launch_predict_bi(hmme_ctx* ctx, const hmme_plane* src, const uint8_t* ref0, const uint8_t* ref1, const int16_t* d_field, const uint8_t* d_dirs, int mv_per_ctu,
                      int first, int count, uint8_t* dst, int dst_pitch, hipStream_t s, const hmme::MePredBiWp<1>* pw = nullptr,
                      const hmme::MePredBiRefs<1>* pr = nullptr, const hmme::MePredBiWp<2>* prw = nullptr) {
  const int n_ctu = hmme_num_ctus(src->width, src->height);
  with_sample_type(src->bps, [&](auto sample) {
    using T = decltype(sample);
    if (mv_per_ctu == 256) {   // unweighted; pr: hmme_predict_bi_refs4_device
      const auto go4 = [&](auto kernel, auto refs) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)count), dim3(256), 0, s, ref0, ref1, src->pitch, d_field, d_dirs, n_ctu, first, src->width, src->height, src->bit_depth, dst,
                           dst_pitch, refs);
      };
      if (pr) go4(hmme::me_predict_bi4_kernel<T, 1>, *pr); else go4(hmme::me_predict_bi4_kernel<T, 0>, hmme::MePredBiRefs<0>{});
      return;
    }
    const auto go = [&](auto kernel, auto wp, auto refs) {
      hipLaunchKernelGGL(kernel, dim3((unsigned)count), dim3(256), 0, s, ref0, ref1, src->pitch, d_field, d_dirs, mv_per_ctu, n_ctu, first, src->width, src->height,
                         src->bit_depth, dst, dst_pitch, wp, refs);
    };
    const hmme::MePredBiWp<0> no_wp;
    const hmme::MePredBiRefs<0> no_refs;
    if (pr && prw) go(hmme::me_predict_bi_kernel<T, 2, 1>, *prw, *pr);
    else if (pr) go(hmme::me_predict_bi_kernel<T, 0, 1>, no_wp, *pr);
    else if (pw) go(hmme::me_predict_bi_kernel<T, 1>, *pw, no_refs);
    else go(hmme::me_predict_bi_kernel<T, 0>, no_wp, no_refs);
  });
  HIP_TRY(ctx, hipGetLastError());
  return HMME_OK;
}
}  // namespace

int hmme_bipred_check(int bit_depth, int refine) {
  char msg[256];
  return bipred_eval(bit_depth, refine, msg, sizeof msg);
}

namespace {
// What hmme_predict_pairs_device, _w_device, hmme_predict_refs_device and _w_device check alike, in the order that decides the code returned
// null_arg: one of the caller's other pointers is null; wps: one weight per plane, or null for none; unit: what a refusal calls plane r
// the MVs-per-CTU test of a predict entry: the *4 family (four) is the 256 layout and nothing else, every other entry takes 1 or 64
bool field_form(int mv_per_ctu, bool four) { return four ? mv_per_ctu == 256 : (mv_per_ctu == 1 || mv_per_ctu == 64); }
struct PredictArgs {
  hmme_frame_params f;   // fp for pairs_begin
  bool identity[hmme::kMaxRefs];
  hmme::MePredWp<1> pw[hmme::kMaxRefs];
};
int predict_args(hmme_ctx* ctx, const char* who, const hmme_plane* const* refs, int n, bool null_arg, const hmme_frame_params* fp, const hmme_weight* wps,
                 const void* d_mv_field, int mv_per_ctu, int out_pitch_bytes, PredictArgs* a, const char* unit = "picture", bool four = false) {
  int rc = bi_check(ctx, who, fp, 0);
  if (rc) return rc;
  if (!refs || null_arg || n < 1 || n > hmme::kMaxRefs) return fail(ctx, HMME_ERR_ARG, "%s: %d pictures outside 1..%d (or a null argument)", who, n, hmme::kMaxRefs);
  for (int r = 0; r < n; ++r) {
    a->identity[r] = true;
    if (!wps) continue;
    char msg[256];
    rc = other_weight_eval(fp->bit_depth, &wps[r], &a->identity[r], &a->pw[r], msg, sizeof msg);
    if (rc) return fail(ctx, rc, "%s: %s %d: %s", who, unit, r, msg);
  }
  if (!d_mv_field || !field_form(mv_per_ctu, four)) return fail(ctx, HMME_ERR_ARG, "%s: null motion field, or %d MVs per CTU (%s)", who, mv_per_ctu, four ? "256" : "1 or 64");
  for (int r = 0; r < n; ++r)
    if (!refs[r]) return fail(ctx, HMME_ERR_ARG, "%s: null plane", who);
  if (out_pitch_bytes < refs[0]->width * refs[0]->bps) return fail(ctx, HMME_ERR_ARG, "%s: output pitch %d below a picture row", who, out_pitch_bytes);
  a->f = *fp;
  a->f.search_range = 1;   // not consulted: nothing is searched
  return HMME_OK;
}

// ---- one body per prediction form, for luma (comps == 1) and for the Cb / Cr of a 4:2:0 picture (comps == 2, with the LUMA width and height) --
// With two components planes, weights and images come in (Cb, Cr) pairs; the fields and the CTU range are those of the luma picture, so the
// planes go through pairs_begin with the whole range (a chroma plane counts its own CTUs) and the luma range is taken from ctu_range.
struct PredictLaunch {
  PairLaunch pl;
  int w = 0, h = 0, n_ctu = 0, first = 0, count = 0;   // luma
  bool acquired = false;                               // the scratch is: pairs_end is due
};
// a refusal of the shared checks names the entry, too
int named(hmme_ctx* ctx, const char* who, int rc) {
  if (rc && ctx->err.compare(0, strlen(who), who) != 0) ctx->err = std::string(who) + ": " + ctx->err;
  return rc;
}
// 4:2:0: an even luma size, every plane (none is null) half of it each way
int chroma_size(hmme_ctx* ctx, const char* who, const hmme_plane* const* planes, int n, int width, int height) {
  if (width < 16 || height < 16 || (width & 1) || (height & 1)) return fail(ctx, HMME_ERR_ARG, "%s: luma size %d x %d: 4:2:0 needs an even size of at least 16 x 16", who, width, height);
  for (int r = 0; r < n; ++r)
    if (planes[r]->width != width / 2 || planes[r]->height != height / 2)
      return fail(ctx, HMME_ERR_ARG, "%s: plane %d is %d x %d, the chroma of a %d x %d picture is %d x %d", who, r, planes[r]->width, planes[r]->height, width, height, width / 2, height / 2);
  return HMME_OK;
}
// after predict_args (no plane is null): pairs_begin -- every plane of this context, of one size, of fp's bit depth, each ordered like a
// reference -- and the luma geometry; for two components behind the planes' size against the luma size and the luma CTU range
int predict_begin(hmme_ctx* ctx, const char* who, const hmme_plane* const* planes, int n, int comps, int width, int height, const hmme_frame_params* fp,
                  const PredictArgs& a, hipStream_t s, PredictLaunch* L) {
  hmme_frame_params f = a.f;
  if (comps == 2) {
    int rc = chroma_size(ctx, who, planes, n, width, height);
    if (rc == HMME_OK) rc = named(ctx, who, ctu_range(ctx, fp, hmme_num_ctus(width, height), &L->first, &L->count));
    if (rc) return rc;
    f.ctu_first = 0; f.ctu_count = -1;
  }
  const int rc = named(ctx, who, pairs_begin(ctx, planes, planes, n, &f, s, &L->pl));
  if (rc) return rc;
  L->acquired = L->pl.count != 0;
  if (comps == 1) { width = planes[0]->width; height = planes[0]->height; L->first = L->pl.first; L->count = L->pl.count; }
  L->w = width; L->h = height; L->n_ctu = hmme_num_ctus(width, height);
  return HMME_OK;
}

extern "C++" {
template <int FORM, int WP>
int launch_chroma(hmme_ctx* ctx, const hmme_plane* p0, const hmme::MeChromaSrc& src, const int16_t* d_field, int mv_per_ctu, const PredictLaunch& cl, void* d_cb, void* d_cr,
                  int out_pitch_bytes, hipStream_t s, const hmme::MeChromaWp<FORM, WP>& wp) {
  with_sample_type(p0->bps, [&](auto sample) {
    using T = decltype(sample);
    const auto go = [&](auto kernel, const auto&... weights) {
      hipLaunchKernelGGL(kernel, dim3((unsigned)cl.count), dim3(256), 0, s, src, p0->pitch, d_field, cl.first, cl.w, cl.h, p0->bit_depth, (uint8_t*)d_cb, (uint8_t*)d_cr,
                         out_pitch_bytes, weights...);
    };
    if constexpr (FORM == 1) {   // the forms with a 4x4 field: hmme_predict_chroma_refs4_device ...
      if (mv_per_ctu == 256) return go(hmme::me_predict_chroma4_kernel<T, WP>, wp);
    }
    if constexpr (FORM == 2 && WP == 0) {   // ... and hmme_predict_chroma_bi4_device (unweighted: its kernel takes no weights)
      if (mv_per_ctu == 256) return go(hmme::me_predict_chroma_bi4_kernel<T>, wp);
    }
    if constexpr (FORM == 3 && WP == 0) {   // ... and hmme_predict_chroma_bi_refs4_device: the same kernel with a reference per block and list
      if (mv_per_ctu == 256) return go(hmme::me_predict_chroma_bi4_kernel<T, 1>, wp);
    }
    if (mv_per_ctu == 1) go(hmme::me_predict_chroma_kernel<T, FORM, WP, 1>, wp); else go(hmme::me_predict_chroma_kernel<T, FORM, WP, 64>, wp);
  });
  HIP_TRY(ctx, hipGetLastError());
  return HMME_OK;
}
}  // extern "C++"

// hmme_predict_pairs_device (wps == null), _w_device and hmme_predict_chroma_pairs_device: one launch per picture; WP = 0 without weights and
// where the picture's are the identity
int predict_pairs(hmme_ctx* ctx, const char* who, const hmme_plane* const* refs, int n_pairs, int comps, int width, int height, const hmme_frame_params* fp,
                  const hmme_weight* wps, const void* d_mv_field, int mv_per_ctu, void* const* d_outs, int out_pitch_bytes, void* stream) {
  const int np = comps * n_pairs;
  PredictArgs a;
  int rc = predict_args(ctx, who, refs, np, !d_outs, fp, wps, d_mv_field, mv_per_ctu, out_pitch_bytes, &a, comps == 2 ? "plane" : "picture");
  if (rc) return rc;
  for (int r = 0; r < np; ++r)
    if (!d_outs[r]) return fail(ctx, HMME_ERR_ARG, "%s: null output image", who);
  hipStream_t s = (hipStream_t)stream;
  PredictLaunch L;
  rc = predict_begin(ctx, who, refs, np, comps, width, height, fp, a, s, &L);
  if (rc || !L.acquired) return rc;
  const size_t field = (size_t)L.n_ctu * mv_per_ctu * 2;
  for (int i = 0; i < n_pairs && rc == HMME_OK && L.count; ++i) {
    const int16_t* f = (const int16_t*)d_mv_field + field * i;
    if (comps == 1) {
      rc = launch_predict(ctx, refs[i], f, mv_per_ctu, L.first, L.count, false, nullptr, 0, (uint8_t*)d_outs[i], 0, 0, out_pitch_bytes, s, a.identity[i] ? nullptr : &a.pw[i]);
      continue;
    }
    hmme::MeChromaSrc src = {};
    src.set.base[0] = refs[2 * i]->origin(); src.set.base[1] = refs[2 * i + 1]->origin();
    if (a.identity[2 * i] && a.identity[2 * i + 1])
      rc = launch_chroma<0, 0>(ctx, refs[0], src, f, mv_per_ctu, L, d_outs[2 * i], d_outs[2 * i + 1], out_pitch_bytes, s, hmme::MeChromaWp<0, 0>{});
    else
      rc = launch_chroma<0, 1>(ctx, refs[0], src, f, mv_per_ctu, L, d_outs[2 * i], d_outs[2 * i + 1], out_pitch_bytes, s, hmme::MeChromaWp<0, 1>{{a.pw[2 * i], a.pw[2 * i + 1]}});
  }
  return pairs_end(ctx, refs, refs, np, s, rc);   // whatever the launches returned: the scratch is acquired
}

// What the _frame forms check before anything is staged.  planes: the n of the call, `comps` per picture; null_arg: one of the caller's other
// pointers is null.  Chroma also answers here for what a luma call leaves to the launch: the images are staged at the first plane's size and
// sample type, so its depth and every plane's size against the luma size are looked at first.
bool frame_null_outs(void* const* outs, int comps) { return !outs || !outs[0] || (comps == 2 && !outs[1]); }
int frame_args(hmme_ctx* ctx, const char* who, const hmme_frame_params* fp, const hmme_plane* const* planes, int n, int comps, bool null_arg, int mv_per_ctu, int width,
               int height, bool four = false) {
  if (!planes || null_arg || !field_form(mv_per_ctu, four))
    return fail(ctx, HMME_ERR_ARG, "%s: null argument, or %d MVs per CTU (%s)", who, mv_per_ctu, four ? "256" : "1 or 64");
  for (int r = 0; r < n; ++r)
    if (!planes[r]) return fail(ctx, HMME_ERR_ARG, "%s: null plane", who);
  if (comps == 1) return HMME_OK;
  if (planes[0]->bit_depth != fp->bit_depth) return fail(ctx, HMME_ERR_ARG, "%s: planes hold %d-bit samples, the call asks for %d", who, planes[0]->bit_depth, fp->bit_depth);
  return chroma_size(ctx, who, planes, n, width, height);
}
// frame_args and the n weights (null: none) of the uni-directional forms.  A luma call answers for a weight before its arguments, a chroma
// call behind them: what each did when it was written, and what tests/test_gpu_predict_refusal_order.py pins.
int frame_checks(hmme_ctx* ctx, const char* who, const hmme_frame_params* fp, const hmme_plane* const* planes, int n, int comps, bool null_arg, int mv_per_ctu, int width,
                 int height, const hmme_weight* wps, const char* unit, bool four = false) {
  int rc = comps == 2 ? frame_args(ctx, who, fp, planes, n, comps, null_arg, mv_per_ctu, width, height, four) : HMME_OK;
  for (int r = 0; rc == HMME_OK && wps && r < n; ++r) {
    char msg[256];
    rc = other_weight_eval(fp->bit_depth, &wps[r], nullptr, nullptr, msg, sizeof msg);
    if (rc) return fail(ctx, rc, "%s: %s %d: %s", who, unit, r, msg);
  }
  if (rc == HMME_OK && comps == 1) rc = frame_args(ctx, who, fp, planes, n, comps, null_arg, mv_per_ctu, width, height, four);
  return rc;
}
// hmme_predict_frame, _w, hmme_predict_refs_frame, hmme_predict_bi_frame and their chroma forms through the staging arena: up go the motion
// field (`lists` of them, one behind the other), the block field (a reference or direction per block; null: none) and the call's `comps`
// images, `launch` gets their device addresses, the images come back: samples that are not written come back as they were.
// comps == 2: p0 is the Cb plane, the fields are those of the LUMA CTUs, and the Cr image has the Cb image's size and stride
int frame_staged(hmme_ctx* ctx, const char* who, const hmme_plane* p0, int comps, int width, int height, const int16_t* mv_field, const uint8_t* block_field, int mv_per_ctu,
                 void* const* outs, int out_stride, int lists, const std::function<int(void*, void*, void* const*, int, hipStream_t)>& launch) {
  if (p0->ctx != ctx) return named(ctx, who, fail(ctx, HMME_ERR_ARG, "plane belongs to another context (planes are used with the context that created them)"));
  if (out_stride < p0->width) return fail(ctx, HMME_ERR_ARG, "%s: output stride %d below the picture width", who, out_stride);
  const size_t blocks = (size_t)(comps == 2 ? hmme_num_ctus(width, height) : p0->n_ctu) * mv_per_ctu, row = (size_t)p0->width * p0->bps;
  Stage st(ctx);
  const int field = st.in(mv_field, sizeof(int16_t) * 2 * blocks * lists), bfield = st.in(block_field, blocks);
  const int img0 = st.image(outs[0], row, p0->height, (size_t)out_stride * p0->bps), img1 = st.image(comps == 2 ? outs[1] : nullptr, row, p0->height, (size_t)out_stride * p0->bps);
  int rc = st.begin();
  if (rc == HMME_OK) {
    void* d_outs[2] = {st.at(img0), st.at(img1)};
    rc = launch(st.at(field), st.at(bfield), d_outs, (int)row, ctx->stream);
  }
  return named(ctx, who, rc ? rc : st.end());
}

// hmme_predict_frame (wps == null), hmme_predict_frame_w and hmme_predict_chroma_frame; refs / wps / outs: `comps` entries
int predict_frame(hmme_ctx* ctx, const char* who, const hmme_plane* const* refs, int comps, int width, int height, const hmme_frame_params* fp, const hmme_weight* wps,
                  const int16_t* mv_field, int mv_per_ctu, void* const* outs, int out_stride) {
  int rc = bi_check(ctx, who, fp, 0);
  if (rc == HMME_OK) rc = frame_checks(ctx, who, fp, refs, comps, comps, !mv_field || frame_null_outs(outs, comps), mv_per_ctu, width, height, wps, comps == 2 ? "plane" : "picture");
  if (rc) return rc;
  return frame_staged(ctx, who, refs[0], comps, width, height, mv_field, nullptr, mv_per_ctu, outs, out_stride, 1, [&](void* d_field, void*, void* const* d_outs, int pitch, hipStream_t s) {
    return predict_pairs(ctx, who, refs, 1, comps, width, height, fp, wps, d_field, mv_per_ctu, d_outs, pitch, s);
  });
}
}  // namespace

int hmme_predict_pairs_device(hmme_ctx* ctx, const hmme_plane* const* refs, int n_pairs, const hmme_frame_params* fp, const void* d_mv_field,
                              int mv_per_ctu, void* const* d_outs, int out_pitch_bytes, void* stream) {
  if (!ctx) return HMME_ERR_ARG;
  return predict_pairs(ctx, "hmme_predict_pairs_device", refs, n_pairs, 1, 0, 0, fp, nullptr, d_mv_field, mv_per_ctu, d_outs, out_pitch_bytes, stream);
}

int hmme_predict_pairs_w_device(hmme_ctx* ctx, const hmme_plane* const* refs, int n_pairs, const hmme_frame_params* fp, const hmme_weight* wps,
                                const void* d_mv_field, int mv_per_ctu, void* const* d_outs, int out_pitch_bytes, void* stream) {
  if (!ctx) return HMME_ERR_ARG;
  if (!wps) return fail(ctx, HMME_ERR_ARG, "hmme_predict_pairs_w_device: null weights");
  return predict_pairs(ctx, "hmme_predict_pairs_w_device", refs, n_pairs, 1, 0, 0, fp, wps, d_mv_field, mv_per_ctu, d_outs, out_pitch_bytes, stream);
}

int hmme_predict_frame(hmme_ctx* ctx, const hmme_plane* ref, const hmme_frame_params* fp, const int16_t* mv_field, int mv_per_ctu, void* out,
                       int out_stride) {
  if (!ctx) return HMME_ERR_ARG;
  return predict_frame(ctx, "hmme_predict_frame", &ref, 1, 0, 0, fp, nullptr, mv_field, mv_per_ctu, &out, out_stride);
}

int hmme_predict_frame_w(hmme_ctx* ctx, const hmme_plane* ref, const hmme_frame_params* fp, const hmme_weight* wp, const int16_t* mv_field,
                         int mv_per_ctu, void* out, int out_stride) {
  if (!ctx) return HMME_ERR_ARG;
  if (!wp) return fail(ctx, HMME_ERR_ARG, "hmme_predict_frame_w: null weight");
  return predict_frame(ctx, "hmme_predict_frame_w", &ref, 1, 0, 0, fp, wp, mv_field, mv_per_ctu, &out, out_stride);
}

namespace {
// The weights of the lists form, in the header's order: 1. the argument errors of all searched weights, then of all other weights; 2. the
// searched lines per reference, with `refine`; 3. the "other weight" line per other reference.  (check_bi_weights goes pair by pair instead.)
int bipred_refs_weight_eval(int bit_depth, const hmme_weight* wps, int n_refs, const hmme_weight* other_wps, int n_others, int refine, BiWp* out, char* msg, size_t n) {
  const hmme_weight* const lists[2] = {wps, other_wps};
  const int cnt[2] = {n_refs, n_others};
  static const char* const name[2] = {"searched", "other"};
  char why[192];
  msg[0] = 0;
  for (int l = 0; l < 2; ++l) {
    if (bit_depth < 8 || bit_depth > 12) { snprintf(msg, n, "bit depth %d outside 8..12", bit_depth); return HMME_ERR_ARG; }
    if (!lists[l]) { snprintf(msg, n, "null weights of the %s list", name[l]); return HMME_ERR_ARG; }
    if (cnt[l] < 1 || cnt[l] > hmme::kMaxRefs) { snprintf(msg, n, "%s list: %d references outside 1..%d", name[l], cnt[l], hmme::kMaxRefs); return HMME_ERR_ARG; }
    for (int r = 0; r < cnt[l]; ++r) {
      const int rc = bi_weight_args(bit_depth, &lists[l][r], name[l], why, sizeof why);
      if (rc) { snprintf(msg, n, "%s reference %d: %s", name[l], r, why); return rc; }
    }
  }
  BiWp bw;
  for (int r = 0; r < n_refs; ++r) {
    const int rc = bi_searched_eval(bit_depth, &wps[r], refine, &bw, r, why, sizeof why);
    if (rc) { snprintf(msg, n, "searched reference %d: %s", r, why); return rc; }
  }
  std::fill_n(bw.bias, n_refs, *std::max_element(bw.bias, bw.bias + n_refs));   // ONE origin, hence ONE bias
  for (int r = 0; r < n_others; ++r) {
    const int rc = bi_other_eval(bit_depth, &other_wps[r], &bw, r, why, sizeof why);
    if (rc) { snprintf(msg, n, "other reference %d: %s", r, why); return rc; }
  }
  if (out) *out = bw;
  return HMME_OK;
}
int check_bi_refs_weights(hmme_ctx* ctx, const char* who, const hmme_frame_params* fp, const hmme_weight* wps, int n_refs, const hmme_weight* other_wps, int n_others,
                          int refine, BiWp* bw) {
  if (!fp) return fail(ctx, HMME_ERR_ARG, "%s: null params", who);
  char msg[256];
  const int rc = bipred_refs_weight_eval(fp->bit_depth, wps, n_refs, other_wps, n_others, refine, bw, msg, sizeof msg);
  return rc ? fail(ctx, rc, "%s: %s", who, msg) : HMME_OK;
}
// bi_args for the lists form
int bi_refs_args(hmme_ctx* ctx, const char* who, const hmme_plane* cur, const hmme_plane* const* refs, int n_refs, const hmme_plane* const* others, int n_others,
                 const hmme_frame_params* fp, const void* d_other_mv, const void* d_other_ref, int mv_per_ctu, bool four = false) {
  if (!cur || !refs || !others || n_refs < 1 || n_refs > hmme::kMaxRefs || n_others < 1 || n_others > hmme::kMaxRefs)
    return fail(ctx, HMME_ERR_ARG, "%s: %d / %d reference pictures outside 1..%d (or a null plane or plane list)", who, n_refs, n_others, hmme::kMaxRefs);
  // the *_bi_refs4 entries (four) are the 256 layout and nothing else; every other entry takes 1 or 64
  if (!d_other_mv || !d_other_ref || (four ? mv_per_ctu != 256 : (mv_per_ctu != 1 && mv_per_ctu != 64)))
    return fail(ctx, HMME_ERR_ARG, "%s: null motion or reference field, or %d MVs per CTU (%s)", who, mv_per_ctu, four ? "256" : "1 or 64");
  for (int r = 0; r < n_refs; ++r)
    if (!refs[r]) return fail(ctx, HMME_ERR_ARG, "%s: null plane", who);
  for (int r = 0; r < n_others; ++r) {
    if (!others[r]) return fail(ctx, HMME_ERR_ARG, "%s: null plane", who);
    if (others[r]->ctx != ctx) return fail(ctx, HMME_ERR_ARG, "plane belongs to another context (planes are used with the context that created them)");
    if (others[r]->width != cur->width || others[r]->height != cur->height) return fail(ctx, HMME_ERR_ARG, "%s: the other list's plane %d differs in size", who, r);
    if (others[r]->bit_depth != fp->bit_depth) return fail(ctx, HMME_ERR_ARG, "%s: the other list's plane %d holds %d-bit samples, the call asks for %d", who, r, others[r]->bit_depth, fp->bit_depth);
  }
  return HMME_OK;
}

// A bi launch of either form, as the bodies take it after its checks
struct BiLaunch {
  const hmme_plane* const* curs;   // the n searched (current, reference) pairs; the lists form gives its one current picture as `cur`,
  const hmme_plane* cur;           //   which bi_call puts into every entry of curs
  const hmme_plane* const* refs;
  int n;
  const hmme_plane* const* others;   // the other list: a plane per pair (n_others == n), or the planes d_other_ref chooses among
  int n_others;
  const void* d_other_mv;            // its motion field(s): int16 [n | 1][n_ctu][mv_per_ctu][2]
  const void* d_other_ref;           // null: the pairs form, one origin per pair; else the lists form, ONE origin for the launch
  int mv_per_ctu;
  const hmme_weight* wps;            // the searched weights; null: no explicit weights
  BiWp bw;
  int origins() const { return d_other_ref ? 1 : n; }
};

// Where the origins 2 * cur - pred + bias go, origin k at dst + slot * k: the CTU blocks a search reads, or the padded plane a refinement
// reads by pitch -- only the CTU blocks are written and read (a partial CTU's block ends 63 samples into the 128 / 80-sample margins at most)
struct BiOrigin {
  uint8_t* dst; size_t slot; long ctu_x, ctu_y; int pitch;
  static BiOrigin blocks(hmme_ctx* ctx, const WpGeom& g, int ctus_x) { return {ctx->wp(1), g.blk_bytes, hmme::kBlkBytes16, (long)ctus_x * hmme::kBlkBytes16, 128}; }
  static BiOrigin plane(hmme_ctx* ctx, const WpGeom& g) { return {ctx->wp(3) + g.origin, g.plane_bytes, 128, 64L * g.pitch, g.pitch}; }
};
// *at: the origin pair r is searched against; it is formed behind the copy of the last pair that reads it -- per pair in the pairs form (it
// depends on the pair's field), once behind the last pair's in the lists form: others[0] gives the geometry all planes share, the weights go
// along unless every other weight is the identity
int bi_origin(hmme_ctx* ctx, const BiLaunch& B, int r, const PairLaunch& pl, const BiOrigin& o, hipStream_t s, const uint8_t** at) {
  const bool lists = B.d_other_ref != nullptr;
  const int k = lists ? 0 : r;
  uint8_t* dst = o.dst + o.slot * k;
  *at = dst;
  if (lists && r != B.n - 1) return HMME_OK;
  if (B.mv_per_ctu == 256) {   // the *_bi4 and *_bi_refs4 entries (unweighted): the origin from one MV per 4x4 block
    const hmme::MePred4Origin<1> org = {B.curs[k]->d_blocks, B.bw.bias[k], o.ctu_x, o.ctu_y};
    RefSet set = one_ref(B.others[k]->origin());   // pairs: the pair's plane; lists: the planes d_other_ref chooses among, per 4x4 block
    for (int q = 0; lists && q < B.n_others; ++q) set.base[q] = B.others[q]->origin();
    return launch_predict4(ctx, B.others[k], set, lists ? B.n_others : 1, (const int16_t*)B.d_other_mv + (size_t)B.curs[0]->n_ctu * 512 * k,
                           lists ? (const uint8_t*)B.d_other_ref : nullptr, pl.first, pl.count, dst, o.pitch, s, nullptr, &org);
  }
  hmme::MePredRefs<1> pr = {one_ref(nullptr), (const uint8_t*)B.d_other_ref, B.n_others};
  for (int q = 0; lists && q < B.n_others; ++q) pr.set.base[q] = B.others[q]->origin();
  const size_t field = (size_t)B.curs[0]->n_ctu * B.mv_per_ctu * 2;
  return launch_predict(ctx, B.others[k], (const int16_t*)B.d_other_mv + field * k, B.mv_per_ctu, pl.first, pl.count, true, B.curs[k]->d_blocks, B.bw.bias[k], dst,
                        o.ctu_x, o.ctu_y, o.pitch, s, lists || B.bw.other_identity[k] ? nullptr : &B.bw.other.ref[k], lists ? &pr : nullptr,
                        lists && !B.bw.others_identity ? &B.bw.other : nullptr);
}
// after the kernels are enqueued: all planes of the launch have a reader on `s`
int bi_end(hmme_ctx* ctx, const BiLaunch& B, hipStream_t s, int rc) {
  if (!B.d_other_ref) return pairs_end(ctx, B.curs, B.refs, B.n, s, rc, B.others);
  const hmme_plane* read[hmme::kMaxRefs + 1] = {B.cur};   // the planes do not come in pairs: the current picture and the searched list, the other list
  std::copy(B.refs, B.refs + B.n, read + 1);
  return lists_end(ctx, read, B.n + 1, B.others, B.n_others, s, rc);
}

// the bi search after its checks (fp->fen is 0 with explicit weights)
int bi_search(hmme_ctx* ctx, const BiLaunch& B, const hmme_frame_params* fp, const void* d_center_q, const void* d_pred_q, void* d_out_mv, void* d_out_sad,
              void* stream) {
  if (!d_out_mv || !d_out_sad) return fail(ctx, HMME_ERR_ARG, "null output buffer");
  hipStream_t s = (hipStream_t)stream;
  PairLaunch pl;
  int rc = pairs_begin(ctx, B.curs, B.refs, B.n, fp, s, &pl);
  if (rc || pl.count == 0) return rc;
  for (int r = 0; r < B.n_others && rc == HMME_OK; ++r) rc = plane_wait(ctx, B.others[r], s);
  const WpGeom g(B.refs[0]);
  const int ctus_x = B.curs[0]->ctus_x;
  if (rc == HMME_OK) rc = ensure(ctx, ctx->buf[kWp0], g.plane_bytes * B.n);
  if (rc == HMME_OK) rc = ensure(ctx, ctx->buf[kWp1], g.blk_bytes * B.origins());
  const BiOrigin o = BiOrigin::blocks(ctx, g, ctus_x);
  RefSet wrefs = one_ref(nullptr), wcurs = one_ref(nullptr);
  CopyCache wref(ctx->wp(0), g.plane_bytes, false);   // the references with the origin's bias
  for (int r = 0; r < B.n && rc == HMME_OK; ++r) {
    const int bias = B.bw.bias[r];   // origin and weighted reference carry the same bias
    rc = cached_copy(ctx, wref, g, r, B.wps ? CopyKey{B.refs[r], B.wps[r].w0, B.wps[r].round, B.wps[r].shift, B.wps[r].offset + bias} : CopyKey{B.refs[r], 1, 0, 0, bias},
                     s, &wrefs.base[r]);
    if (rc == HMME_OK) rc = bi_origin(ctx, B, r, pl, o, s, &wcurs.base[r]);
  }
  const FramePlan plan = plan_launch(ctx, fp, pl.count, B.n, true);
  if (rc == HMME_OK) rc = prep_jobs(ctx, B.curs[0], fp, d_pred_q, pl.first, pl.count, B.n, s, plan, d_center_q);
  if (rc == HMME_OK) rc = run_search(ctx, wcurs, ctus_x, wrefs, g.pitch, fp, plan, (int16_t*)d_out_mv, (uint32_t*)d_out_sad, s);
  return bi_end(ctx, B, s, rc);
}

// the bi refinement after its checks: one launch per run of equal searched weights, one launch in all without explicit weights
int bi_refine(hmme_ctx* ctx, const BiLaunch& B, const hmme_frame_params* fp, const void* d_center_q, const void* d_pred_q, const void* d_int_mv, int use_hadamard,
              void* d_out_qmv, void* d_out_cost, void* stream) {
  if (!d_int_mv || !d_out_qmv || !d_out_cost) return fail(ctx, HMME_ERR_ARG, "null buffer");
  hipStream_t s = (hipStream_t)stream;
  PairLaunch pl;
  int rc = pairs_begin(ctx, B.curs, B.refs, B.n, fp, s, &pl);
  if (rc || pl.count == 0) return rc;
  for (int r = 0; r < B.n_others && rc == HMME_OK; ++r) rc = plane_wait(ctx, B.others[r], s);
  const int src_wide = B.curs[0]->bps == 2 ? 1 : 0, n_ctu = B.curs[0]->n_ctu;
  const WpGeom g(B.refs[0]);
  if (rc == HMME_OK && !src_wide) rc = ensure(ctx, ctx->buf[kWp2], g.plane_bytes * B.n);
  if (rc == HMME_OK) rc = ensure(ctx, ctx->buf[kWp3], g.plane_bytes * B.origins());
  const BiOrigin o = BiOrigin::plane(ctx, g);
  RefSet c = one_ref(nullptr), rf = one_ref(nullptr);
  CopyCache raw(ctx->wp(2), g.plane_bytes, false);
  for (int r = 0; r < B.n && rc == HMME_OK; ++r) {
    // the RAW reference is interpolated: a u16 plane serves as it is, an 8-bit one is widened
    if (src_wide) rf.base[r] = pl.refs.base[r];
    else rc = cached_copy(ctx, raw, g, r, CopyKey{B.refs[r], 1, 0, 0, 0}, s, &rf.base[r]);
    if (rc == HMME_OK) rc = bi_origin(ctx, B, r, pl, o, s, &c.base[r]);
  }
  for (int a = 0, b; a < B.n && rc == HMME_OK; a = b) {
    b = run_end(B.wps, a, B.n);
    RefSet ca = one_ref(nullptr), ra = one_ref(nullptr);
    for (int r = a; r < b; ++r) { ca.base[r - a] = c.base[r]; ra.base[r - a] = rf.base[r]; }
    // the run's own table and counter in the same buffer as the run before (on one stream: behind its kernel)
    const size_t res0 = (size_t)a * pl.count * HMME_NUM_CTU_PARTS;
    RefineLaunch L;
    refine_common(L, pl, B.curs[0], fp, use_hadamard, (const int16_t*)d_int_mv + 2 * res0, (int16_t*)d_out_qmv + 2 * res0, (uint32_t*)d_out_cost + res0);
    L.curs = ca; L.refs = ra; L.cur_pitch = g.pitch; L.ref_pitch = g.pitch;
    L.build.wide = 1; L.build.wp = 1;
    L.fw = frac_wp(B.wps && !B.bw.identity[a] ? &B.wps[a] : nullptr, B.bw.bias[a]);   // (an identity weight: the weight is 1)
    L.d_pred = d_pred_q ? (const int16_t*)d_pred_q + (size_t)a * n_ctu * 2 : nullptr;
    L.d_center = d_center_q ? (const int16_t*)d_center_q + (size_t)a * n_ctu * 2 : nullptr;
    L.pairs = b - a;
    L.table = FracTable::kAlways;   // the table carries the window centres (FracPrep derives windows from predictors only)
    rc = launch_refine(ctx, L, s);
  }
  return bi_end(ctx, B, s, rc);
}

// What distinguishes the sixteen entries: the name for messages, the form, explicit weights or not, search or refinement, and whether the
// arrays are the host's (the synchronous forms).  plain: the unweighted device entry, which an all-identity call IS and answers as
enum : unsigned { kBiLists = 1, kBiWeighted = 2, kBiRefine = 4, kBiHost = 8, kBiFour = 16 };   // kBiFour: the field is the 256 layout (either form, unweighted)
struct BiCall {
  const char* who; const char* plain; bool lists, weighted, refine, host, four;
  BiCall(const char* who_, unsigned what, const char* plain_ = nullptr)
      : who(who_), plain(plain_), lists(what & kBiLists), weighted(what & kBiWeighted), refine(what & kBiRefine), host(what & kBiHost), four(what & kBiFour) {}
};

// The refusals of a bi call in the order that decides the code returned: null params, then the weights (without them: the depth), then the
// arguments pairs_begin does not look at.  Leaves in B the summary of the weights and in *f the parameters the bodies run with
int bi_checks(hmme_ctx* ctx, const BiCall& c, BiLaunch* B, const hmme_frame_params* fp, const hmme_weight* other_wps, hmme_frame_params* f) {
  const char* who = c.who;
  int rc;
  if (!c.weighted) rc = bi_check(ctx, who, fp, c.refine);
  else if (c.lists) rc = check_bi_refs_weights(ctx, who, fp, B->wps, B->n, other_wps, B->n_others, c.refine, &B->bw);
  else rc = check_bi_weights(ctx, who, fp, B->wps, other_wps, B->n, c.refine, &B->bw);
  if (rc) return rc;
  *f = *fp;
  if (c.weighted) f->fen = 0;   // xGetSADw reads every row (TComRdCost.cpp:467-469): FEN is not consulted
  if (c.weighted && B->bw.all_identity) { B->wps = nullptr; if (!c.host) who = c.plain; }
  if (!B->wps) B->bw = BiWp::unweighted(f->bit_depth);
  return c.lists ? bi_refs_args(ctx, who, B->cur, B->refs, B->n, B->others, B->n_others, f, B->d_other_mv, B->d_other_ref, B->mv_per_ctu, c.four)
                 : bi_args(ctx, who, B->curs, B->refs, B->others, B->n, f, B->d_other_mv, B->mv_per_ctu, c.four);
}

// Every entry: the checks, then the body on the caller's stream -- or, for the host arrays of a synchronous form, through the staging arena
// on ctx->stream: up go the field, the reference field (lists), the centres and stage_in's items, the tables come back
int bi_call(hmme_ctx* ctx, const BiCall& c, BiLaunch B, const hmme_frame_params* fp, const hmme_weight* other_wps, const void* center_q, const void* pred_q,
            const void* int_mv, int use_hadamard, void* out_mv, void* out_cost, void* stream) {
  if (!ctx) return HMME_ERR_ARG;
  const hmme_plane* same[hmme::kMaxRefs];
  if (c.lists) { std::fill_n(same, hmme::kMaxRefs, B.cur); B.curs = same; }
  hmme_frame_params f;
  int rc = bi_checks(ctx, c, &B, fp, other_wps, &f);   // (a synchronous form: before anything is staged)
  if (rc) return rc;
  const auto body = [&](const void* d_center, const void* d_pred, const void* d_imv, void* d_mv, void* d_cost, void* on) {
    return c.refine ? bi_refine(ctx, B, &f, d_center, d_pred, d_imv, use_hadamard, d_mv, d_cost, on) : bi_search(ctx, B, &f, d_center, d_pred, d_mv, d_cost, on);
  };
  if (!c.host) return body(center_q, pred_q, int_mv, out_mv, out_cost, stream);
  int count;
  Stage st(ctx);
  FrameItems it;
  const size_t n_ctu = (size_t)B.curs[0]->n_ctu, blocks = n_ctu * B.mv_per_ctu;
  const int field = st.in(B.d_other_mv, sizeof(int16_t) * 2 * blocks), rfield = st.in(B.d_other_ref, blocks);
  const int center = st.in(center_q, sizeof(int16_t) * 2 * n_ctu * B.n);
  rc = stage_in(ctx, B.curs[0], B.refs[0], fp, B.n, (const int16_t*)pred_q, c.refine, (const int16_t*)int_mv, (int16_t*)out_mv, (uint32_t*)out_cost, &count, st, &it);
  if (rc || count == 0) return rc;
  B.d_other_mv = st.at(field); B.d_other_ref = st.at(rfield);
  rc = body(st.at(center), st.at(it.pred), st.at(it.imv), st.at(it.mv), st.at(it.cost), ctx->stream);
  return rc ? rc : st.end();
}
}  // namespace

int hmme_bipred_weight_check(int bit_depth, const hmme_weight* wp, const hmme_weight* other_wp, int refine) {
  char msg[256];
  return bipred_weight_eval(bit_depth, wp, other_wp, refine, nullptr, 0, msg, sizeof msg);
}

int hmme_bipred_refs_weight_check(int bit_depth, const hmme_weight* wps, int n_refs, const hmme_weight* other_wps, int n_others, int refine) {
  char msg[256];
  return bipred_refs_weight_eval(bit_depth, wps, n_refs, other_wps, n_others, refine, nullptr, msg, sizeof msg);
}

// the pairs form on device arrays ...
int hmme_search_pairs_bi_device(hmme_ctx* ctx, const hmme_plane* const* curs, const hmme_plane* const* refs, const hmme_plane* const* others,
                                int n_pairs, const hmme_frame_params* fp, const void* d_other_mv, int mv_per_ctu, const void* d_center_q,
                                const void* d_pred_q, void* d_out_mv, void* d_out_sad, void* stream) {
  return bi_call(ctx, BiCall("hmme_search_pairs_bi_device", 0), {curs, nullptr, refs, n_pairs, others, n_pairs, d_other_mv, nullptr, mv_per_ctu},
                 fp, nullptr, d_center_q, d_pred_q, nullptr, 0, d_out_mv, d_out_sad, stream);
}

int hmme_refine_pairs_bi_device(hmme_ctx* ctx, const hmme_plane* const* curs, const hmme_plane* const* refs, const hmme_plane* const* others,
                                int n_pairs, const hmme_frame_params* fp, const void* d_other_mv, int mv_per_ctu, const void* d_center_q,
                                const void* d_pred_q, const void* d_int_mv, int use_hadamard, void* d_out_qmv, void* d_out_cost, void* stream) {
  return bi_call(ctx, BiCall("hmme_refine_pairs_bi_device", kBiRefine), {curs, nullptr, refs, n_pairs, others, n_pairs, d_other_mv, nullptr, mv_per_ctu},
                 fp, nullptr, d_center_q, d_pred_q, d_int_mv, use_hadamard, d_out_qmv, d_out_cost, stream);
}

int hmme_search_pairs_bi_w_device(hmme_ctx* ctx, const hmme_plane* const* curs, const hmme_plane* const* refs, const hmme_plane* const* others,
                                  int n_pairs, const hmme_frame_params* fp, const hmme_weight* wps, const hmme_weight* other_wps, const void* d_other_mv,
                                  int mv_per_ctu, const void* d_center_q, const void* d_pred_q, void* d_out_mv, void* d_out_sad, void* stream) {
  return bi_call(ctx, BiCall("hmme_search_pairs_bi_w_device", kBiWeighted, "hmme_search_pairs_bi_device"),
                 {curs, nullptr, refs, n_pairs, others, n_pairs, d_other_mv, nullptr, mv_per_ctu, wps}, fp, other_wps, d_center_q, d_pred_q, nullptr, 0, d_out_mv, d_out_sad,
                 stream);
}

int hmme_refine_pairs_bi_w_device(hmme_ctx* ctx, const hmme_plane* const* curs, const hmme_plane* const* refs, const hmme_plane* const* others,
                                  int n_pairs, const hmme_frame_params* fp, const hmme_weight* wps, const hmme_weight* other_wps, const void* d_other_mv,
                                  int mv_per_ctu, const void* d_center_q, const void* d_pred_q, const void* d_int_mv, int use_hadamard, void* d_out_qmv,
                                  void* d_out_cost, void* stream) {
  return bi_call(ctx, BiCall("hmme_refine_pairs_bi_w_device", kBiWeighted | kBiRefine, "hmme_refine_pairs_bi_device"),
                 {curs, nullptr, refs, n_pairs, others, n_pairs, d_other_mv, nullptr, mv_per_ctu, wps}, fp, other_wps, d_center_q, d_pred_q, d_int_mv, use_hadamard, d_out_qmv,
                 d_out_cost, stream);
}

// ... from one MV per 4x4 block (the rule: include/hmme.h, "B pictures from one MV per 4x4 block"): every refusal names the entry, those of
// the shared checks (the CTU range, plane ownership, a null table), too ...
int hmme_search_pairs_bi4_device(hmme_ctx* ctx, const hmme_plane* const* curs, const hmme_plane* const* refs, const hmme_plane* const* others,
                                 int n_pairs, const hmme_frame_params* fp, const void* d_other_mv, const void* d_center_q, const void* d_pred_q,
                                 void* d_out_mv, void* d_out_sad, void* stream) {
  if (!ctx) return HMME_ERR_ARG;
  return named(ctx, "hmme_search_pairs_bi4_device", bi_call(ctx, BiCall("hmme_search_pairs_bi4_device", kBiFour), {curs, nullptr, refs, n_pairs, others, n_pairs, d_other_mv, nullptr, 256},
                 fp, nullptr, d_center_q, d_pred_q, nullptr, 0, d_out_mv, d_out_sad, stream));
}

int hmme_refine_pairs_bi4_device(hmme_ctx* ctx, const hmme_plane* const* curs, const hmme_plane* const* refs, const hmme_plane* const* others,
                                 int n_pairs, const hmme_frame_params* fp, const void* d_other_mv, const void* d_center_q, const void* d_pred_q,
                                 const void* d_int_mv, int use_hadamard, void* d_out_qmv, void* d_out_cost, void* stream) {
  if (!ctx) return HMME_ERR_ARG;
  return named(ctx, "hmme_refine_pairs_bi4_device", bi_call(ctx, BiCall("hmme_refine_pairs_bi4_device", kBiFour | kBiRefine), {curs, nullptr, refs, n_pairs, others, n_pairs, d_other_mv, nullptr, 256},
                 fp, nullptr, d_center_q, d_pred_q, d_int_mv, use_hadamard, d_out_qmv, d_out_cost, stream));
}

int hmme_search_frame_bi4(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* ref, const hmme_plane* other, const hmme_frame_params* fp,
                          const int16_t* other_mv, const int16_t* center_q, const int16_t* pred_q, int16_t* out_mv, uint32_t* out_sad) {
  if (!ctx) return HMME_ERR_ARG;
  return named(ctx, "hmme_search_frame_bi4", bi_call(ctx, BiCall("hmme_search_frame_bi4", kBiFour | kBiHost), {&cur, nullptr, &ref, 1, &other, 1, other_mv, nullptr, 256}, fp, nullptr, center_q,
                 pred_q, nullptr, 0, out_mv, out_sad, nullptr));
}

int hmme_refine_frame_bi4(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* ref, const hmme_plane* other, const hmme_frame_params* fp,
                          const int16_t* other_mv, const int16_t* center_q, const int16_t* pred_q, const int16_t* int_mv, int use_hadamard,
                          int16_t* out_qmv, uint32_t* out_cost) {
  if (!ctx) return HMME_ERR_ARG;
  return named(ctx, "hmme_refine_frame_bi4", bi_call(ctx, BiCall("hmme_refine_frame_bi4", kBiFour | kBiRefine | kBiHost), {&cur, nullptr, &ref, 1, &other, 1, other_mv, nullptr, 256}, fp, nullptr,
                 center_q, pred_q, int_mv, use_hadamard, out_qmv, out_cost, nullptr));
}

// ... and one pair of it on host arrays
int hmme_search_frame_bi(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* ref, const hmme_plane* other, const hmme_frame_params* fp,
                         const int16_t* other_mv, int mv_per_ctu, const int16_t* center_q, const int16_t* pred_q, int16_t* out_mv, uint32_t* out_sad) {
  return bi_call(ctx, BiCall("hmme_search_frame_bi", kBiHost), {&cur, nullptr, &ref, 1, &other, 1, other_mv, nullptr, mv_per_ctu}, fp, nullptr, center_q,
                 pred_q, nullptr, 0, out_mv, out_sad, nullptr);
}

int hmme_refine_frame_bi(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* ref, const hmme_plane* other, const hmme_frame_params* fp,
                         const int16_t* other_mv, int mv_per_ctu, const int16_t* center_q, const int16_t* pred_q, const int16_t* int_mv,
                         int use_hadamard, int16_t* out_qmv, uint32_t* out_cost) {
  return bi_call(ctx, BiCall("hmme_refine_frame_bi", kBiRefine | kBiHost), {&cur, nullptr, &ref, 1, &other, 1, other_mv, nullptr, mv_per_ctu}, fp, nullptr, center_q,
                 pred_q, int_mv, use_hadamard, out_qmv, out_cost, nullptr);
}

int hmme_search_frame_bi_w(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* ref, const hmme_plane* other, const hmme_frame_params* fp,
                           const hmme_weight* wp, const hmme_weight* other_wp, const int16_t* other_mv, int mv_per_ctu, const int16_t* center_q,
                           const int16_t* pred_q, int16_t* out_mv, uint32_t* out_sad) {
  return bi_call(ctx, BiCall("hmme_search_frame_bi_w", kBiWeighted | kBiHost), {&cur, nullptr, &ref, 1, &other, 1, other_mv, nullptr, mv_per_ctu, wp}, fp, other_wp,
                 center_q, pred_q, nullptr, 0, out_mv, out_sad, nullptr);
}

int hmme_refine_frame_bi_w(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* ref, const hmme_plane* other, const hmme_frame_params* fp,
                           const hmme_weight* wp, const hmme_weight* other_wp, const int16_t* other_mv, int mv_per_ctu, const int16_t* center_q,
                           const int16_t* pred_q, const int16_t* int_mv, int use_hadamard, int16_t* out_qmv, uint32_t* out_cost) {
  return bi_call(ctx, BiCall("hmme_refine_frame_bi_w", kBiWeighted | kBiRefine | kBiHost), {&cur, nullptr, &ref, 1, &other, 1, other_mv, nullptr, mv_per_ctu, wp}, fp, other_wp,
                 center_q, pred_q, int_mv, use_hadamard, out_qmv, out_cost, nullptr);
}

// the lists form on device arrays ...
int hmme_search_frame_bi_refs_device(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* const* refs, int n_refs, const hmme_plane* const* others,
                                     int n_others, const hmme_frame_params* fp, const void* d_other_mv, const void* d_other_ref, int mv_per_ctu,
                                     const void* d_center_q, const void* d_pred_q, void* d_out_mv, void* d_out_sad, void* stream) {
  return bi_call(ctx, BiCall("hmme_search_frame_bi_refs_device", kBiLists), {nullptr, cur, refs, n_refs, others, n_others, d_other_mv, d_other_ref, mv_per_ctu},
                 fp, nullptr, d_center_q, d_pred_q, nullptr, 0, d_out_mv, d_out_sad, stream);
}

int hmme_refine_frame_bi_refs_device(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* const* refs, int n_refs, const hmme_plane* const* others,
                                     int n_others, const hmme_frame_params* fp, const void* d_other_mv, const void* d_other_ref, int mv_per_ctu,
                                     const void* d_center_q, const void* d_pred_q, const void* d_int_mv, int use_hadamard, void* d_out_qmv, void* d_out_cost,
                                     void* stream) {
  return bi_call(ctx, BiCall("hmme_refine_frame_bi_refs_device", kBiLists | kBiRefine), {nullptr, cur, refs, n_refs, others, n_others, d_other_mv, d_other_ref, mv_per_ctu},
                 fp, nullptr, d_center_q, d_pred_q, d_int_mv, use_hadamard, d_out_qmv, d_out_cost, stream);
}

int hmme_search_frame_bi_refs_w_device(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* const* refs, int n_refs, const hmme_plane* const* others,
                                       int n_others, const hmme_frame_params* fp, const hmme_weight* wps, const hmme_weight* other_wps, const void* d_other_mv,
                                       const void* d_other_ref, int mv_per_ctu, const void* d_center_q, const void* d_pred_q, void* d_out_mv, void* d_out_sad,
                                       void* stream) {
  return bi_call(ctx, BiCall("hmme_search_frame_bi_refs_w_device", kBiLists | kBiWeighted, "hmme_search_frame_bi_refs_device"),
                 {nullptr, cur, refs, n_refs, others, n_others, d_other_mv, d_other_ref, mv_per_ctu, wps}, fp, other_wps, d_center_q, d_pred_q, nullptr, 0, d_out_mv, d_out_sad,
                 stream);
}

int hmme_refine_frame_bi_refs_w_device(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* const* refs, int n_refs, const hmme_plane* const* others,
                                       int n_others, const hmme_frame_params* fp, const hmme_weight* wps, const hmme_weight* other_wps, const void* d_other_mv,
                                       const void* d_other_ref, int mv_per_ctu, const void* d_center_q, const void* d_pred_q, const void* d_int_mv, int use_hadamard,
                                       void* d_out_qmv, void* d_out_cost, void* stream) {
  return bi_call(ctx, BiCall("hmme_refine_frame_bi_refs_w_device", kBiLists | kBiWeighted | kBiRefine, "hmme_refine_frame_bi_refs_device"),
                 {nullptr, cur, refs, n_refs, others, n_others, d_other_mv, d_other_ref, mv_per_ctu, wps}, fp, other_wps, d_center_q, d_pred_q, d_int_mv, use_hadamard, d_out_qmv,
                 d_out_cost, stream);
}

// ... and on host arrays
int hmme_search_frame_bi_refs(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* const* refs, int n_refs, const hmme_plane* const* others, int n_others,
                              const hmme_frame_params* fp, const int16_t* other_mv, const uint8_t* other_ref, int mv_per_ctu, const int16_t* center_q,
                              const int16_t* pred_q, int16_t* out_mv, uint32_t* out_sad) {
  return bi_call(ctx, BiCall("hmme_search_frame_bi_refs", kBiLists | kBiHost), {nullptr, cur, refs, n_refs, others, n_others, other_mv, other_ref, mv_per_ctu}, fp,
                 nullptr, center_q, pred_q, nullptr, 0, out_mv, out_sad, nullptr);
}

int hmme_refine_frame_bi_refs(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* const* refs, int n_refs, const hmme_plane* const* others, int n_others,
                              const hmme_frame_params* fp, const int16_t* other_mv, const uint8_t* other_ref, int mv_per_ctu, const int16_t* center_q,
                              const int16_t* pred_q, const int16_t* int_mv, int use_hadamard, int16_t* out_qmv, uint32_t* out_cost) {
  return bi_call(ctx, BiCall("hmme_refine_frame_bi_refs", kBiLists | kBiRefine | kBiHost), {nullptr, cur, refs, n_refs, others, n_others, other_mv, other_ref, mv_per_ctu}, fp,
                 nullptr, center_q, pred_q, int_mv, use_hadamard, out_qmv, out_cost, nullptr);
}

int hmme_search_frame_bi_refs_w(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* const* refs, int n_refs, const hmme_plane* const* others, int n_others,
                                const hmme_frame_params* fp, const hmme_weight* wps, const hmme_weight* other_wps, const int16_t* other_mv, const uint8_t* other_ref,
                                int mv_per_ctu, const int16_t* center_q, const int16_t* pred_q, int16_t* out_mv, uint32_t* out_sad) {
  return bi_call(ctx, BiCall("hmme_search_frame_bi_refs_w", kBiLists | kBiWeighted | kBiHost),
                 {nullptr, cur, refs, n_refs, others, n_others, other_mv, other_ref, mv_per_ctu, wps}, fp, other_wps, center_q, pred_q, nullptr, 0, out_mv, out_sad, nullptr);
}

int hmme_refine_frame_bi_refs_w(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* const* refs, int n_refs, const hmme_plane* const* others, int n_others,
                                const hmme_frame_params* fp, const hmme_weight* wps, const hmme_weight* other_wps, const int16_t* other_mv, const uint8_t* other_ref,
                                int mv_per_ctu, const int16_t* center_q, const int16_t* pred_q, const int16_t* int_mv, int use_hadamard, int16_t* out_qmv,
                                uint32_t* out_cost) {
  return bi_call(ctx, BiCall("hmme_refine_frame_bi_refs_w", kBiLists | kBiWeighted | kBiRefine | kBiHost),
                 {nullptr, cur, refs, n_refs, others, n_others, other_mv, other_ref, mv_per_ctu, wps}, fp, other_wps, center_q, pred_q, int_mv, use_hadamard, out_qmv, out_cost,
                 nullptr);
}

// ... and from one MV and one reference index per 4x4 block (the rule: include/hmme.h, "B pictures with several references per list from one MV
// per 4x4 block"): unweighted, the 256 layout and nothing else; every refusal names the entry
int hmme_search_frame_bi_refs4_device(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* const* refs, int n_refs, const hmme_plane* const* others,
                                      int n_others, const hmme_frame_params* fp, const void* d_other_mv, const void* d_other_ref, const void* d_center_q,
                                      const void* d_pred_q, void* d_out_mv, void* d_out_sad, void* stream) {
  if (!ctx) return HMME_ERR_ARG;
  return named(ctx, "hmme_search_frame_bi_refs4_device", bi_call(ctx, BiCall("hmme_search_frame_bi_refs4_device", kBiLists | kBiFour),
                 {nullptr, cur, refs, n_refs, others, n_others, d_other_mv, d_other_ref, 256}, fp, nullptr, d_center_q, d_pred_q, nullptr, 0, d_out_mv, d_out_sad, stream));
}

int hmme_refine_frame_bi_refs4_device(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* const* refs, int n_refs, const hmme_plane* const* others,
                                      int n_others, const hmme_frame_params* fp, const void* d_other_mv, const void* d_other_ref, const void* d_center_q,
                                      const void* d_pred_q, const void* d_int_mv, int use_hadamard, void* d_out_qmv, void* d_out_cost, void* stream) {
  if (!ctx) return HMME_ERR_ARG;
  return named(ctx, "hmme_refine_frame_bi_refs4_device", bi_call(ctx, BiCall("hmme_refine_frame_bi_refs4_device", kBiLists | kBiFour | kBiRefine),
                 {nullptr, cur, refs, n_refs, others, n_others, d_other_mv, d_other_ref, 256}, fp, nullptr, d_center_q, d_pred_q, d_int_mv, use_hadamard, d_out_qmv, d_out_cost,
                 stream));
}

int hmme_search_frame_bi_refs4(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* const* refs, int n_refs, const hmme_plane* const* others, int n_others,
                               const hmme_frame_params* fp, const int16_t* other_mv, const uint8_t* other_ref, const int16_t* center_q, const int16_t* pred_q,
                               int16_t* out_mv, uint32_t* out_sad) {
  if (!ctx) return HMME_ERR_ARG;
  return named(ctx, "hmme_search_frame_bi_refs4", bi_call(ctx, BiCall("hmme_search_frame_bi_refs4", kBiLists | kBiFour | kBiHost),
                 {nullptr, cur, refs, n_refs, others, n_others, other_mv, other_ref, 256}, fp, nullptr, center_q, pred_q, nullptr, 0, out_mv, out_sad, nullptr));
}

int hmme_refine_frame_bi_refs4(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* const* refs, int n_refs, const hmme_plane* const* others, int n_others,
                               const hmme_frame_params* fp, const int16_t* other_mv, const uint8_t* other_ref, const int16_t* center_q, const int16_t* pred_q,
                               const int16_t* int_mv, int use_hadamard, int16_t* out_qmv, uint32_t* out_cost) {
  if (!ctx) return HMME_ERR_ARG;
  return named(ctx, "hmme_refine_frame_bi_refs4", bi_call(ctx, BiCall("hmme_refine_frame_bi_refs4", kBiLists | kBiFour | kBiRefine | kBiHost),
                 {nullptr, cur, refs, n_refs, others, n_others, other_mv, other_ref, 256}, fp, nullptr, center_q, pred_q, int_mv, use_hadamard, out_qmv, out_cost, nullptr));
}

// ---- the selection calls: partition decision and motion field from the 593-slot tables, over one table set per picture pair
// (hmme_select_pairs_device / _frame), the references of a picture (hmme_select_refs_*), the two lists of a B picture (hmme_select_dirs_*)
// and the references of its two lists (hmme_select_dirs_refs_*).  Every entry fills in a SelectCall; select_device checks and launches it,
// select_host stages its arrays around select_device.  The entries of the last three families stand further down, by their predictions -------
namespace {
constexpr int kMaxDirPics = 4;
// the evaluation of each family's parameters: what its hmme_select_*check entry returns and what its launches refuse with
int select_eval(const hmme_select_params* p, char* msg, size_t cap) {
  msg[0] = 0;
  if (!p) { snprintf(msg, cap, "null parameters"); return HMME_ERR_ARG; }
  if (p->mv_per_ctu != 64 && p->mv_per_ctu != 256) { snprintf(msg, cap, "%d MVs per CTU (64 or 256)", p->mv_per_ctu); return HMME_ERR_ARG; }
  if ((p->mv_unit != 0 && p->mv_unit != 1) || (p->price_mv != 0 && p->price_mv != 1)) {
    snprintf(msg, cap, "mv_unit %d / price_mv %d (each 0 or 1)", p->mv_unit, p->price_mv);
    return HMME_ERR_ARG;
  }
  if (!(p->part_mask & 1u) || (p->part_mask & ~0xf7u)) { snprintf(msg, cap, "part_mask 0x%x: bit 0 must be set, only bits 0, 1, 2, 4..7 exist", p->part_mask); return HMME_ERR_ARG; }
  if (p->min_depth < 0 || p->max_depth > 3 || p->min_depth > p->max_depth) { snprintf(msg, cap, "depths %d..%d (0 <= min <= max <= 3)", p->min_depth, p->max_depth); return HMME_ERR_ARG; }
  if (p->cu_cost > (1u << 20) || p->pu_cost > (1u << 20)) { snprintf(msg, cap, "cu_cost %u / pu_cost %u above 2^20", p->cu_cost, p->pu_cost); return HMME_ERR_ARG; }
  return HMME_OK;
}
// ... of a decision over n_pics pictures x n_refs references (the decision of one table set per picture pair: n_refs = 1, no prices)
int select_refs_eval(const hmme_select_params* sel, int n_pics, int n_refs, const uint32_t* ref_cost, char* msg, size_t cap) {
  const int bad = select_eval(sel, msg, cap);
  if (bad) return bad;
  if (n_refs < 1 || n_refs > hmme::kMaxRefs) { snprintf(msg, cap, "%d reference pictures outside 1..%d", n_refs, hmme::kMaxRefs); return HMME_ERR_ARG; }
  if (n_pics < 1 || (long long)n_pics * n_refs > hmme::kMaxRefs) {
    snprintf(msg, cap, "%d pictures x %d references: outside 1..%d table sets", n_pics, n_refs, hmme::kMaxRefs);
    return HMME_ERR_ARG;
  }
  for (int r = 0; ref_cost && r < n_refs; ++r)
    if (ref_cost[r] > (1u << 20)) { snprintf(msg, cap, "ref_cost[%d] = %u above 2^20", r, ref_cost[r]); return HMME_ERR_ARG; }
  return HMME_OK;
}
// ... of both B-picture decisions, up to the bit counts: dirs = the caller's hmme_dir_params or hmme_dir_refs_params, for null only
// per: the layout the entry decides at -- 64, or 256 for hmme_select_dirs4_*
int select_bi_eval(const hmme_select_params* sel, int n_pics, const void* dirs, char* msg, size_t cap, int per = 64) {
  const int bad = select_eval(sel, msg, cap);
  if (bad) return bad;
  if (sel->mv_per_ctu != per || sel->mv_unit != 0 || sel->price_mv != 0) {
    snprintf(msg, cap, "mv_per_ctu %d, mv_unit %d, price_mv %d: the direction is decided on quarter-pel refinement tables, one MV per %s block (%d, 0, 0)",
             sel->mv_per_ctu, sel->mv_unit, sel->price_mv, per == 64 ? "8x8" : "4x4", per);
    return HMME_ERR_ARG;
  }
  if (n_pics < 1 || n_pics > kMaxDirPics) { snprintf(msg, cap, "%d pictures outside 1..%d", n_pics, kMaxDirPics); return HMME_ERR_ARG; }
  if (!dirs) { snprintf(msg, cap, "null direction parameters"); return HMME_ERR_ARG; }
  return HMME_OK;
}
int select_dirs_eval(const hmme_select_params* sel, int n_pics, const hmme_dir_params* dirs, char* msg, size_t cap, int per = 64) {
  const int bad = select_bi_eval(sel, n_pics, dirs, msg, cap, per);
  if (bad) return bad;
  for (int p = 0; p < n_pics; ++p) {
    const uint32_t v[5] = {dirs[p].dir_bits[0], dirs[p].dir_bits[1], dirs[p].dir_bits[2], dirs[p].list_bits[0], dirs[p].list_bits[1]};
    for (int k = 0; k < 5; ++k)
      if (v[k] > 4096) { snprintf(msg, cap, "picture %d: %s[%d] = %u above 4096", p, k < 3 ? "dir_bits" : "list_bits", k < 3 ? k : k - 3, v[k]); return HMME_ERR_ARG; }
  }
  return HMME_OK;
}
int select_dirs_refs_eval(const hmme_select_params* sel, int n_pics, int n_refs_max, const hmme_dir_refs_params* dirs, char* msg, size_t cap, int per = 64) {
  const int bad = select_bi_eval(sel, n_pics, dirs, msg, cap, per);
  if (bad) return bad;
  if (n_refs_max < 1 || n_refs_max > hmme::kMaxDirRefs) { snprintf(msg, cap, "%d table sets per list outside 1..%d", n_refs_max, hmme::kMaxDirRefs); return HMME_ERR_ARG; }
  for (int p = 0; p < n_pics; ++p) {
    const hmme_dir_refs_params& d = dirs[p];
    for (int k = 0; k < 3; ++k)
      if (d.dir_bits[k] > 4096) { snprintf(msg, cap, "picture %d: dir_bits[%d] = %u above 4096", p, k, d.dir_bits[k]); return HMME_ERR_ARG; }
    for (int l = 0; l < 2; ++l) {
      if (d.n_refs[l] < 1 || d.n_refs[l] > n_refs_max) { snprintf(msg, cap, "picture %d: %d references in list %d outside 1..%d", p, d.n_refs[l], l, n_refs_max); return HMME_ERR_ARG; }
      for (int r = 0; r < hmme::kMaxDirRefs; ++r)
        if (d.ref_bits[l][r] > 4096) { snprintf(msg, cap, "picture %d: ref_bits[%d][%d] = %u above 4096", p, l, r, d.ref_bits[l][r]); return HMME_ERR_ARG; }
    }
    if (d.l1_valid_mask >> d.n_refs[1]) { snprintf(msg, cap, "picture %d: l1_valid_mask 0x%x names references at or above %d", p, d.l1_valid_mask, d.n_refs[1]); return HMME_ERR_ARG; }
  }
  return HMME_OK;
}

// One selection call, device or host form.  The buffers in the order they are checked: the family's own, then the ones every family has
// kSelectDirs4 / kSelectDirsRefs4: kSelectDirs / kSelectDirsRefs at one MV per 4x4 block
enum SelectFamily { kSelectTable, kSelectRefs, kSelectDirs, kSelectDirsRefs, kSelectDirs4, kSelectDirsRefs4 };
enum SelectBufName { kMvBi, kCostBi, kUniField, kUniRef, kOutRef, kOutDir, kMv, kCost, kPredQ, kOutField, kOutSlot, kOutCost, kSelectBufs };
enum SelectRole { kInTable, kInPicture, kOut };   // an input over the CTUs of the range / of the picture; an output (of the picture: the range is written)
struct SelectBuf {
  const char* name;
  SelectRole role;
  size_t ctu_bytes;   // per CTU of one part
  size_t parts;       // table sets or lists, one behind the other; 0: the family has no such buffer
  unsigned align;     // of a device address: what the kernel's widest access to it needs
  bool required;      // may not be null
  const void* p;      // device address or host array
};
struct SelectCall {
  const char* who;    // the entry the caller made: every refusal but ctu_range's names it
  SelectFamily family;
  int width, height, n_pics;
  int n_refs;         // kSelectRefs: references per picture; kSelectDirsRefs: table sets per list (n_refs_max)
  const hmme_frame_params* fp;
  const hmme_select_params* sel;
  const uint32_t* ref_cost = nullptr;                // kSelectRefs (null: zeros)
  const hmme_dir_params* dirs = nullptr;             // kSelectDirs, kSelectDirs4
  const hmme_dir_refs_params* dir_refs = nullptr;    // kSelectDirsRefs, kSelectDirsRefs4
  SelectBuf buf[kSelectBufs];
  SelectCall(const char* who, SelectFamily family, int width, int height, int n_pics, int n_refs, const hmme_frame_params* fp, const hmme_select_params* sel)
      : who(who), family(family), width(width), height(height), n_pics(n_pics), n_refs(n_refs), fp(fp), sel(sel) {
    const bool refs = family == kSelectRefs, bi = family >= kSelectDirs, multi = family == kSelectDirsRefs || family == kSelectDirsRefs4;
    const bool four = family == kSelectDirs4 || family == kSelectDirsRefs4;
    // (sizes matter to select_host alone, behind the evaluation of sel and n_refs)
    const size_t per = sel ? (size_t)sel->mv_per_ctu : 0, row = HMME_NUM_CTU_PARTS * 4, none = 0, one = 1, lists = bi ? 2 : 1;
    const size_t sets = refs ? (size_t)n_refs : multi ? 2 * (size_t)n_refs : lists;
    const size_t bper = four ? 256 : 64;   // blocks per CTU of a B-picture decision's own buffers
    const SelectBuf all[kSelectBufs] = {
        {"bi MV table", kInTable, row, bi ? sets : none, 4, true, nullptr},
        {"bi cost table", kInTable, row, bi ? sets : none, 4, true, nullptr},
        {"input field", kInPicture, bper * 4, bi ? lists : none, 4, true, nullptr},
        {"input reference", kInPicture, bper, multi ? lists : none, 1, true, nullptr},
        {"reference", kOut, refs ? per : bper, refs ? one : multi ? lists : none, refs || four ? 2u : 1u, true, nullptr},   // with four MVs per 8x8 block the kernel stores two indices at a time
        {"direction", kOut, bper, bi ? one : none, multi && !four ? 1u : 2u, true, nullptr},   // kSelectDirs4, kSelectDirsRefs4: two directions per store
        {"MV table", kInTable, row, sets, 4, true, nullptr},   // the kernels move MVs as dwords
        {"cost table", kInTable, row, sets, 4, true, nullptr},
        {"predictor", kInPicture, 4, sets, 2, false, nullptr},
        {"field", kOut, per * 4, lists, 8, true, nullptr},     // with four MVs per 8x8 block, two entries per store
        {"slot", kOut, per * 2, one, 4, false, nullptr},
        {"CTU cost", kOut, 4, one, 4, false, nullptr}};
    for (int b = 0; b < kSelectBufs; ++b) buf[b] = all[b];
  }
  SelectCall& with(SelectBufName b, const void* p) { buf[b].p = p; return *this; }
  SelectCall& with(const uint32_t* prices) { ref_cost = prices; return *this; }
  SelectCall& with(const hmme_dir_params* d) { dirs = d; return *this; }
  SelectCall& with(const hmme_dir_refs_params* d) { dir_refs = d; return *this; }
};

// parameters, then null and (device) misaligned buffers, then the CTU range
int select_check(hmme_ctx* ctx, const SelectCall& c, bool device, int* n_ctu, int* first, int* count) {
  if (!ctx) return HMME_ERR_ARG;
  const auto buffers = [&](int lo, int hi) {   // of the buffers [lo, hi): a null one, then a misaligned one
    for (int b = lo; b < hi; ++b)
      if (c.buf[b].parts && c.buf[b].required && !c.buf[b].p) return fail(ctx, HMME_ERR_ARG, "%s: null %s %s", c.who, c.buf[b].name, device ? "buffer" : "array");
    for (int b = lo; device && b < hi; ++b)
      if ((uintptr_t)c.buf[b].p & (c.buf[b].align - 1)) return fail(ctx, HMME_ERR_ARG, "%s: misaligned %s buffer (%u bytes)", c.who, c.buf[b].name, c.buf[b].align);
    return (int)HMME_OK;
  };
  char msg[256];
  int bad;
  if (c.family == kSelectRefs && (bad = buffers(kOutRef, kOutRef + 1))) return bad;   // hmme_select_refs_* look at the reference buffer before the parameters
  if (c.family == kSelectDirs) bad = select_dirs_eval(c.sel, c.n_pics, c.dirs, msg, sizeof msg);
  else if (c.family == kSelectDirs4) bad = select_dirs_eval(c.sel, c.n_pics, c.dirs, msg, sizeof msg, 256);
  else if (c.family == kSelectDirsRefs) bad = select_dirs_refs_eval(c.sel, c.n_pics, c.n_refs, c.dir_refs, msg, sizeof msg);
  else if (c.family == kSelectDirsRefs4) bad = select_dirs_refs_eval(c.sel, c.n_pics, c.n_refs, c.dir_refs, msg, sizeof msg, 256);
  else bad = select_refs_eval(c.sel, c.n_pics, c.n_refs, c.ref_cost, msg, sizeof msg);
  if (bad) return fail(ctx, bad, "%s: %s", c.who, msg);
  if ((bad = buffers(0, kMv))) return bad;   // the family's own buffers, then the frame and the buffers every family has
  if (!c.fp || c.width < 1 || c.height < 1) return fail(ctx, HMME_ERR_ARG, "%s: null frame parameters, or a %d x %d picture", c.who, c.width, c.height);
  if ((bad = buffers(kMv, kSelectBufs))) return bad;
  *n_ctu = hmme_num_ctus(c.width, c.height);
  return ctu_range(ctx, c.fp, *n_ctu, first, count);
}

// the *_device entries: the checks, then the family's kernel over the CTUs of the range of every picture
int select_device(hmme_ctx* ctx, const SelectCall& c, hipStream_t stream) {
  int n_ctu, first, count;
  const int rc = select_check(ctx, c, true, &n_ctu, &first, &count);
  if (rc || count == 0) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const hmme_select_params& s = *c.sel;
  const hmme::MeSelect a = {s.mv_per_ctu, s.mv_unit, s.price_mv, s.part_mask, s.min_depth, s.max_depth, s.cu_cost, s.pu_cost};
  const dim3 grid((unsigned)((count + 3) / 4), (unsigned)c.n_pics), block(256);
  const auto tab = [&](SelectBufName b) { return (const uint32_t*)c.buf[b].p; };
  const auto bytes = [&](SelectBufName b) { return (uint8_t*)c.buf[b].p; };
  const int16_t* pred_q = (const int16_t*)c.buf[kPredQ].p;
  uint32_t *out_field = (uint32_t*)c.buf[kOutField].p, *out_cost = (uint32_t*)c.buf[kOutCost].p;
  uint16_t* out_slot = (uint16_t*)c.buf[kOutSlot].p;
  // the kernels take hmme_dir_params and hmme_dir_refs_params member for member: copied below as they are
  using KB = hmme::MeDirBits; using KR = hmme::MeDirRefsBits;
  static_assert(sizeof(KB) == sizeof(hmme_dir_params) && offsetof(KB, list_bits) == offsetof(hmme_dir_params, list_bits), "MeDirBits");
  static_assert(sizeof(KR) == sizeof(hmme_dir_refs_params) && offsetof(KR, n_refs) == offsetof(hmme_dir_refs_params, n_refs) &&
                offsetof(KR, ref_bits) == offsetof(hmme_dir_refs_params, ref_bits) && offsetof(KR, l1_valid_mask) == offsetof(hmme_dir_refs_params, l1_valid_mask) &&
                sizeof(KR::ref_bits) == sizeof(hmme_dir_refs_params::ref_bits), "MeDirRefsBits");
  if (c.family == kSelectTable) {
    hipLaunchKernelGGL(hmme::me_select_kernel, grid, block, 0, stream, tab(kMv), tab(kCost), pred_q, out_field, out_slot, out_cost, a, c.width, c.height, n_ctu, first, count, ctx->lambda_q16);
  } else if (c.family == kSelectRefs) {
    hmme::MeRefCost price = {};
    for (int r = 0; c.ref_cost && r < c.n_refs; ++r) price.c[r] = c.ref_cost[r];
    hipLaunchKernelGGL(hmme::me_select_refs_kernel, grid, block, 0, stream, tab(kMv), tab(kCost), pred_q, out_field, bytes(kOutRef), out_slot, out_cost, a, price, c.n_refs, c.width, c.height,
                       n_ctu, first, count, ctx->lambda_q16);
  } else if (c.family == kSelectDirs || c.family == kSelectDirs4) {
    hmme::MeDirParams bits = {};
    memcpy(bits.p, c.dirs, c.n_pics * sizeof *c.dirs);
    const auto go = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, block, 0, stream, tab(kMv), tab(kCost), tab(kMvBi), tab(kCostBi), tab(kUniField), pred_q, out_field, bytes(kOutDir), out_slot, out_cost, a,
                         bits, c.width, c.height, n_ctu, first, count, ctx->lambda_q16);
    };
    if (c.family == kSelectDirs4) go(hmme::me_select_dirs_kernel<true>); else go(hmme::me_select_dirs_kernel<false>);
  } else {
    hmme::MeDirRefsParams bits = {};
    memcpy(bits.p, c.dir_refs, c.n_pics * sizeof *c.dir_refs);
    const auto go = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, block, 0, stream, tab(kMv), tab(kCost), tab(kMvBi), tab(kCostBi), tab(kUniField), (const uint8_t*)bytes(kUniRef), pred_q, out_field,
                         bytes(kOutRef), bytes(kOutDir), out_slot, out_cost, a, bits, c.n_refs, c.width, c.height, n_ctu, first, count, ctx->lambda_q16);
    };
    if (c.family == kSelectDirsRefs4) go(hmme::me_select_dirs_refs_kernel<true>); else go(hmme::me_select_dirs_refs_kernel<false>);
  }
  HIP_TRY(ctx, hipGetLastError());
  return HMME_OK;
}

// the *_frame entries (one picture): every array the caller passed into the staging arena, select_device on the staged addresses (null where
// the caller's array is), then of the outputs the CTUs of the range back: the caller's entries outside it keep their values
int select_host(hmme_ctx* ctx, const SelectCall& c) {
  int n_ctu, first, count;
  int rc = select_check(ctx, c, false, &n_ctu, &first, &count);   // before anything is staged
  if (rc || count == 0) return rc;
  Stage st(ctx);
  for (const SelectBuf& s : c.buf) {   // item b of the arena is buffer b
    if (s.role == kOut) st.out((void*)s.p, n_ctu * s.ctu_bytes, first * s.ctu_bytes, count * s.ctu_bytes, s.parts);
    else st.in(s.p, s.parts * (s.role == kInTable ? count : n_ctu) * s.ctu_bytes);
  }
  rc = st.begin();
  if (rc == HMME_OK) {
    SelectCall staged = c;
    for (int b = 0; b < kSelectBufs; ++b) staged.buf[b].p = st.at(b);
    rc = select_device(ctx, staged, ctx->stream);
  }
  return rc ? rc : st.end();
}
}  // namespace

int hmme_select_check(const hmme_select_params* sel) {
  char msg[256];
  return select_eval(sel, msg, sizeof msg);
}

int hmme_select_pairs_device(hmme_ctx* ctx, int width, int height, int n_pairs, const hmme_frame_params* fp, const hmme_select_params* sel,
                             const void* d_mv, const void* d_cost, const void* d_pred_q, void* d_out_field, void* d_out_slot, void* d_out_cost,
                             void* stream) {
  return select_device(ctx, SelectCall("hmme_select_pairs_device", kSelectTable, width, height, n_pairs, 1, fp, sel).with(kMv, d_mv).with(kCost, d_cost)
                           .with(kPredQ, d_pred_q).with(kOutField, d_out_field).with(kOutSlot, d_out_slot).with(kOutCost, d_out_cost), (hipStream_t)stream);
}

int hmme_select_frame(hmme_ctx* ctx, int width, int height, const hmme_frame_params* fp, const hmme_select_params* sel, const int16_t* mv,
                      const uint32_t* cost, const int16_t* pred_q, int16_t* out_field, uint16_t* out_slot, uint32_t* out_cost) {
  return select_host(ctx, SelectCall("hmme_select_frame", kSelectTable, width, height, 1, 1, fp, sel).with(kMv, mv).with(kCost, cost).with(kPredQ, pred_q)
                         .with(kOutField, out_field).with(kOutSlot, out_slot).with(kOutCost, out_cost));
}

// ---- residual and per-PU / per-CU distortion of a prediction (the rule: include/hmme.h) -------------------------------------------------------
namespace {
extern "C++" {
template <typename T>
void launch_residual(dim3 grid, hipStream_t s, int per, bool had, bool map, const hmme::RefSet& blocks, const hmme::RefSet& preds, int pred_pitch, const uint16_t* d_slot,
                     const hmme::MeResidualSet& resid, int resid_pitch, uint32_t* d_pu, uint32_t* d_cu, uint32_t* d_ctu, const hmme_plane* p0, int first) {
  const auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, blocks, preds, pred_pitch, d_slot, resid, resid_pitch, d_pu, d_cu, d_ctu, p0->width, p0->height, p0->bit_depth,
                       p0->n_ctu, first);
  };
  const auto with_map = [&](auto per_c, auto had_c) {
    if (map) go(hmme::me_residual_kernel<T, decltype(per_c)::value, decltype(had_c)::value, true>);
    else go(hmme::me_residual_kernel<T, decltype(per_c)::value, decltype(had_c)::value, false>);
  };
  const auto with_had = [&](auto per_c) {
    if (had) with_map(per_c, std::true_type{}); else with_map(per_c, std::false_type{});
  };
  if (per == 64) with_had(std::integral_constant<int, 64>{}); else with_had(std::integral_constant<int, 256>{});
}
}  // extern "C++"
}  // namespace

int hmme_residual_pairs_device(hmme_ctx* ctx, const hmme_plane* const* curs, const void* const* d_preds, int pred_pitch_bytes, int n_pairs,
                               const hmme_frame_params* fp, const void* d_slot, int mv_per_ctu, int use_hadamard, void* const* d_out_resid,
                               int resid_pitch_bytes, void* d_out_pu, void* d_out_cu, void* d_out_ctu, void* stream) {
  if (!ctx) return HMME_ERR_ARG;
  const char* who = "hmme_residual_pairs_device";
  if (!curs || !d_preds || !fp || n_pairs < 1 || n_pairs > hmme::kMaxRefs)
    return fail(ctx, HMME_ERR_ARG, "%s: %d picture pairs outside 1..%d (or a null argument)", who, n_pairs, hmme::kMaxRefs);
  if ((mv_per_ctu != 64 && mv_per_ctu != 256) || (use_hadamard != 0 && use_hadamard != 1))
    return fail(ctx, HMME_ERR_ARG, "%s: %d blocks per CTU (64 or 256), use_hadamard %d (0 or 1)", who, mv_per_ctu, use_hadamard);
  if (!d_out_resid && !d_out_pu && !d_out_cu && !d_out_ctu) return fail(ctx, HMME_ERR_ARG, "%s: no output", who);
  hmme::RefSet preds = {};
  hmme::MeResidualSet resid = {};
  for (int r = 0; r < n_pairs; ++r) {
    if (!curs[r] || !d_preds[r]) return fail(ctx, HMME_ERR_ARG, "%s: null plane or predicted image", who);
    if (curs[r]->ctx != ctx) return fail(ctx, HMME_ERR_ARG, "%s: plane belongs to another context (planes are used with the context that created them)", who);
    if (curs[r]->bit_depth != fp->bit_depth) return fail(ctx, HMME_ERR_ARG, "%s: planes hold %d-bit samples, the call asks for %d", who, curs[r]->bit_depth, fp->bit_depth);
    preds.base[r] = (const uint8_t*)d_preds[r];
    resid.base[r] = d_out_resid ? (uint8_t*)d_out_resid[r] : nullptr;
    if (((uintptr_t)preds.base[r] & 3) || ((uintptr_t)resid.base[r] & 7)) return fail(ctx, HMME_ERR_ARG, "%s: misaligned image (predicted 4 bytes, residual 8)", who);
  }
  const hmme_plane* p0 = curs[0];
  if (pred_pitch_bytes < p0->width * p0->bps) return fail(ctx, HMME_ERR_ARG, "%s: predicted pitch %d below a picture row", who, pred_pitch_bytes);
  if (d_out_resid && (resid_pitch_bytes < p0->width * 2 || (resid_pitch_bytes & 7)))
    return fail(ctx, HMME_ERR_ARG, "%s: residual pitch %d below a picture row of int16, or no multiple of 8", who, resid_pitch_bytes);
  if (((uintptr_t)d_slot & 3) || ((uintptr_t)d_out_pu & 3) || ((uintptr_t)d_out_cu & 3) || ((uintptr_t)d_out_ctu & 3))
    return fail(ctx, HMME_ERR_ARG, "%s: misaligned buffer (slots and the uint32 outputs 4 bytes)", who);
  hmme_frame_params f = *fp;
  f.search_range = 1;   // not consulted: nothing is searched
  hipStream_t s = (hipStream_t)stream;
  PairLaunch pl;
  int rc = named(ctx, who, pairs_begin(ctx, curs, curs, n_pairs, &f, s, &pl));   // one size, the CTU range; ordered behind the planes' fills
  if (rc || pl.count == 0) return rc;
  const dim3 grid((unsigned)pl.count, (unsigned)n_pairs);
  with_sample_type(p0->bps, [&](auto sample) {
    launch_residual<decltype(sample)>(grid, s, mv_per_ctu, use_hadamard != 0, d_slot != nullptr, pl.cur_blocks, preds, pred_pitch_bytes, (const uint16_t*)d_slot, resid,
                                      resid_pitch_bytes, (uint32_t*)d_out_pu, (uint32_t*)d_out_cu, (uint32_t*)d_out_ctu, p0, pl.first);
  });
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) rc = fail(ctx, HMME_ERR_DEVICE, "%s: launch -> %s", who, hipGetErrorString(e));
  return pairs_end(ctx, curs, curs, n_pairs, s, rc);
}

int hmme_residual_frame(hmme_ctx* ctx, const hmme_plane* cur, const hmme_frame_params* fp, const void* pred, int pred_stride, const uint16_t* slot,
                        int mv_per_ctu, int use_hadamard, int16_t* out_resid, int resid_stride, uint32_t* out_pu, uint32_t* out_cu, uint32_t* out_ctu) {
  if (!ctx) return HMME_ERR_ARG;
  const char* who = "hmme_residual_frame";
  if (!cur || !fp || !pred) return fail(ctx, HMME_ERR_ARG, "%s: null argument", who);
  if ((mv_per_ctu != 64 && mv_per_ctu != 256) || (use_hadamard != 0 && use_hadamard != 1))
    return fail(ctx, HMME_ERR_ARG, "%s: %d blocks per CTU (64 or 256), use_hadamard %d (0 or 1)", who, mv_per_ctu, use_hadamard);
  if (cur->ctx != ctx) return fail(ctx, HMME_ERR_ARG, "%s: plane belongs to another context (planes are used with the context that created them)", who);
  if (pred_stride < cur->width || (out_resid && resid_stride < cur->width))
    return fail(ctx, HMME_ERR_ARG, "%s: stride %d / %d below the picture width", who, pred_stride, resid_stride);
  int first, count;
  int rc = named(ctx, who, ctu_range(ctx, fp, cur->n_ctu, &first, &count));
  if (rc || count == 0) return rc;
  const size_t n_ctu = cur->n_ctu, per = mv_per_ctu, row = (size_t)cur->width * cur->bps, rrow = (size_t)cur->width * 2, rpitch = (rrow + 7) & ~(size_t)7;
  Stage st(ctx);
  const int i_pred = st.image_in(pred, row, cur->height, (size_t)pred_stride * cur->bps), i_slot = st.in(slot, n_ctu * per * 2);
  const int i_res = st.image(out_resid, rrow, cur->height, (size_t)resid_stride * 2, rpitch);
  // only the CTUs of the range come back: the caller's entries outside it keep their values
  const int o_pu = st.out(out_pu, n_ctu * per * 4, first * per * 4, count * per * 4), o_cu = st.out(out_cu, n_ctu * per * 4, first * per * 4, count * per * 4);
  const int o_ctu = st.out(out_ctu, n_ctu * 8, (size_t)first * 8, (size_t)count * 8);
  rc = st.begin();
  if (rc == HMME_OK) {
    const void* d_pred = st.at(i_pred);
    void* d_res = st.at(i_res);
    rc = hmme_residual_pairs_device(ctx, &cur, &d_pred, (int)row, 1, fp, st.at(i_slot), mv_per_ctu, use_hadamard, out_resid ? &d_res : nullptr, (int)rpitch, st.at(o_pu),
                                    st.at(o_cu), st.at(o_ctu), ctx->stream);
    if (rc && ctx->err.compare(0, strlen("hmme_residual_pairs_device"), "hmme_residual_pairs_device") == 0)
      ctx->err.replace(0, strlen("hmme_residual_pairs_device"), who);   // the refusal names the entry the caller made
  }
  return rc ? rc : st.end();
}

// ---- reference picture per PU: the decision over all references' tables, and the prediction that follows it ---------------------------------
int hmme_ref_idx_bits(int n_refs, int ref_idx) {   // TEncSearch.cpp:3030-3037
  if (n_refs < 1 || n_refs > hmme::kMaxRefs || ref_idx < 0 || ref_idx >= n_refs) return -1;
  if (n_refs == 1) return 0;
  return ref_idx + 1 - (ref_idx == n_refs - 1 ? 1 : 0);
}

int hmme_select_refs_check(const hmme_select_params* sel, int n_pics, int n_refs, const uint32_t* ref_cost) {
  char msg[256];
  return select_refs_eval(sel, n_pics, n_refs, ref_cost, msg, sizeof msg);
}

int hmme_select_refs_device(hmme_ctx* ctx, int width, int height, int n_pics, int n_refs, const hmme_frame_params* fp, const hmme_select_params* sel,
                            const uint32_t* ref_cost, const void* d_mv, const void* d_cost, const void* d_pred_q, void* d_out_field, void* d_out_ref,
                            void* d_out_slot, void* d_out_cost, void* stream) {
  return select_device(ctx, SelectCall("hmme_select_refs_device", kSelectRefs, width, height, n_pics, n_refs, fp, sel).with(ref_cost).with(kMv, d_mv).with(kCost, d_cost)
                           .with(kPredQ, d_pred_q).with(kOutField, d_out_field).with(kOutRef, d_out_ref).with(kOutSlot, d_out_slot).with(kOutCost, d_out_cost),
                       (hipStream_t)stream);
}

int hmme_select_refs_frame(hmme_ctx* ctx, int width, int height, int n_refs, const hmme_frame_params* fp, const hmme_select_params* sel,
                           const uint32_t* ref_cost, const int16_t* mv, const uint32_t* cost, const int16_t* pred_q, int16_t* out_field, uint8_t* out_ref,
                           uint16_t* out_slot, uint32_t* out_cost) {
  return select_host(ctx, SelectCall("hmme_select_refs_frame", kSelectRefs, width, height, 1, n_refs, fp, sel).with(ref_cost).with(kMv, mv).with(kCost, cost)
                         .with(kPredQ, pred_q).with(kOutField, out_field).with(kOutRef, out_ref).with(kOutSlot, out_slot).with(kOutCost, out_cost));
}

namespace {
// hmme_predict_refs_device (wps == null), _w_device and hmme_predict_chroma_refs_device: ONE launch, every block from the plane (pair) its
// reference index names.  WP = 0 without weights and where every weight is the identity, else 2: every block through addWeightUni with its
// plane's weight (for an identity weight that is the unweighted sample: nested floors).  d_out_cr: the second image of comps == 2
// four: hmme_predict_refs4_device and hmme_predict_chroma_refs4_device -- mv_per_ctu is 256, the reference field may be null (every block
// index 0), and the kernels are me_predict4_kernel / me_predict_chroma4_kernel
int predict_refs(hmme_ctx* ctx, const char* who, const hmme_plane* const* refs, int n_refs, int comps, int width, int height, const hmme_frame_params* fp,
                 const hmme_weight* wps, const void* d_mv_field, const void* d_ref_field, int mv_per_ctu, void* d_out, void* d_out_cr, int out_pitch_bytes, void* stream,
                 bool four = false) {
  const int np = comps * n_refs;
  PredictArgs a;
  int rc = predict_args(ctx, who, refs, np, (!four && !d_ref_field) || !d_out || (comps == 2 && !d_out_cr), fp, wps, d_mv_field, mv_per_ctu, out_pitch_bytes, &a,
                        comps == 2 ? "plane" : "reference", four);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  PredictLaunch L;
  rc = predict_begin(ctx, who, refs, np, comps, width, height, fp, a, s, &L);
  if (rc || !L.acquired) return rc;
  if (L.count) {
    hmme::MePredWp<2> prw = {};
    hmme::MeChromaWp<1, 2> cprw = {};
    bool weighted = false;
    for (int r = 0; r < np; ++r) {
      weighted = weighted || !a.identity[r];
      if (wps) prw.ref[r] = cprw.ref[r] = a.pw[r];
    }
    if (comps == 1 && four) {
      rc = launch_predict4(ctx, refs[0], L.pl.refs, n_refs, (const int16_t*)d_mv_field, (const uint8_t*)d_ref_field, L.first, L.count, (uint8_t*)d_out, out_pitch_bytes, s,
                           weighted ? &prw : nullptr);
    } else if (comps == 1) {
      const hmme::MePredRefs<1> pr = {L.pl.refs, (const uint8_t*)d_ref_field, n_refs};
      rc = launch_predict(ctx, refs[0], (const int16_t*)d_mv_field, mv_per_ctu, L.first, L.count, false, nullptr, 0, (uint8_t*)d_out, 0, 0, out_pitch_bytes, s, nullptr, &pr,
                          weighted ? &prw : nullptr);
    } else {
      const hmme::MeChromaSrc src = {L.pl.refs, (const uint8_t*)d_ref_field, n_refs, L.n_ctu};
      if (weighted) rc = launch_chroma<1, 2>(ctx, refs[0], src, (const int16_t*)d_mv_field, mv_per_ctu, L, d_out, d_out_cr, out_pitch_bytes, s, cprw);
      else rc = launch_chroma<1, 0>(ctx, refs[0], src, (const int16_t*)d_mv_field, mv_per_ctu, L, d_out, d_out_cr, out_pitch_bytes, s, hmme::MeChromaWp<1, 0>{});
    }
  }
  return pairs_end(ctx, refs, refs, np, s, rc);   // whatever the launch returned: the scratch is acquired
}

// hmme_predict_refs_frame (wps == null), _w_frame and hmme_predict_chroma_refs_frame; four: hmme_predict_refs4_frame and
// hmme_predict_chroma_refs4_frame, as in predict_refs
int predict_refs_frame(hmme_ctx* ctx, const char* who, const hmme_plane* const* refs, int n_refs, int comps, int width, int height, const hmme_frame_params* fp,
                       const hmme_weight* wps, const int16_t* mv_field, const uint8_t* ref_field, int mv_per_ctu, void* const* outs, int out_stride, bool four = false) {
  int rc = bi_check(ctx, who, fp, 0);
  if (rc) return rc;
  if (!refs || n_refs < 1 || comps * n_refs > hmme::kMaxRefs || !refs[0])
    return fail(ctx, HMME_ERR_ARG, "%s: %d reference pictures outside 1..%d (or a null plane)", who, n_refs, hmme::kMaxRefs / comps);
  rc = frame_checks(ctx, who, fp, refs, comps * n_refs, comps, !mv_field || (!four && !ref_field) || frame_null_outs(outs, comps), mv_per_ctu, width, height, wps,
                    comps == 2 ? "plane" : "reference", four);
  if (rc) return rc;
  // blocks without a reference, too, come back as they were
  return frame_staged(ctx, who, refs[0], comps, width, height, mv_field, ref_field, mv_per_ctu, outs, out_stride, 1, [&](void* d_field, void* d_ref_field, void* const* d_outs, int pitch, hipStream_t s) {
    return predict_refs(ctx, who, refs, n_refs, comps, width, height, fp, wps, d_field, d_ref_field, mv_per_ctu, d_outs[0], comps == 2 ? d_outs[1] : nullptr, pitch, s, four);
  });
}
}  // namespace

int hmme_predict_refs_device(hmme_ctx* ctx, const hmme_plane* const* refs, int n_refs, const hmme_frame_params* fp, const void* d_mv_field,
                             const void* d_ref_field, int mv_per_ctu, void* d_out, int out_pitch_bytes, void* stream) {
  if (!ctx) return HMME_ERR_ARG;
  return predict_refs(ctx, "hmme_predict_refs_device", refs, n_refs, 1, 0, 0, fp, nullptr, d_mv_field, d_ref_field, mv_per_ctu, d_out, nullptr, out_pitch_bytes, stream);
}

int hmme_predict_refs_w_device(hmme_ctx* ctx, const hmme_plane* const* refs, int n_refs, const hmme_frame_params* fp, const hmme_weight* wps,
                               const void* d_mv_field, const void* d_ref_field, int mv_per_ctu, void* d_out, int out_pitch_bytes, void* stream) {
  if (!ctx) return HMME_ERR_ARG;
  if (!wps) return fail(ctx, HMME_ERR_ARG, "hmme_predict_refs_w_device: null weights");
  return predict_refs(ctx, "hmme_predict_refs_w_device", refs, n_refs, 1, 0, 0, fp, wps, d_mv_field, d_ref_field, mv_per_ctu, d_out, nullptr, out_pitch_bytes, stream);
}

int hmme_predict_refs_frame(hmme_ctx* ctx, const hmme_plane* const* refs, int n_refs, const hmme_frame_params* fp, const int16_t* mv_field,
                            const uint8_t* ref_field, int mv_per_ctu, void* out, int out_stride) {
  if (!ctx) return HMME_ERR_ARG;
  return predict_refs_frame(ctx, "hmme_predict_refs_frame", refs, n_refs, 1, 0, 0, fp, nullptr, mv_field, ref_field, mv_per_ctu, &out, out_stride);
}

int hmme_predict_refs_w_frame(hmme_ctx* ctx, const hmme_plane* const* refs, int n_refs, const hmme_frame_params* fp, const hmme_weight* wps,
                              const int16_t* mv_field, const uint8_t* ref_field, int mv_per_ctu, void* out, int out_stride) {
  if (!ctx) return HMME_ERR_ARG;
  if (!wps) return fail(ctx, HMME_ERR_ARG, "hmme_predict_refs_w_frame: null weights");
  return predict_refs_frame(ctx, "hmme_predict_refs_w_frame", refs, n_refs, 1, 0, 0, fp, wps, mv_field, ref_field, mv_per_ctu, &out, out_stride);
}

// ---- prediction from one MV per 4x4 block: the refs forms on the 256 layout, weights and the reference field optional ---------------------
int hmme_predict_refs4_device(hmme_ctx* ctx, const hmme_plane* const* refs, int n_refs, const hmme_frame_params* fp, const hmme_weight* wps,
                              const void* d_mv_field, const void* d_ref_field, void* d_out, int out_pitch_bytes, void* stream) {
  if (!ctx) return HMME_ERR_ARG;
  return predict_refs(ctx, "hmme_predict_refs4_device", refs, n_refs, 1, 0, 0, fp, wps, d_mv_field, d_ref_field, 256, d_out, nullptr, out_pitch_bytes, stream, true);
}

int hmme_predict_refs4_frame(hmme_ctx* ctx, const hmme_plane* const* refs, int n_refs, const hmme_frame_params* fp, const hmme_weight* wps,
                             const int16_t* mv_field, const uint8_t* ref_field, void* out, int out_stride) {
  if (!ctx) return HMME_ERR_ARG;
  return predict_refs_frame(ctx, "hmme_predict_refs4_frame", refs, n_refs, 1, 0, 0, fp, wps, mv_field, ref_field, 256, &out, out_stride, true);
}

int hmme_predict_chroma_refs4_device(hmme_ctx* ctx, const hmme_plane* const* refs, int n_refs, int width, int height, const hmme_frame_params* fp,
                                     const hmme_weight* wps, const void* d_mv_field, const void* d_ref_field, void* d_out_cb, void* d_out_cr, int out_pitch_bytes,
                                     void* stream) {
  if (!ctx) return HMME_ERR_ARG;
  return predict_refs(ctx, "hmme_predict_chroma_refs4_device", refs, n_refs, 2, width, height, fp, wps, d_mv_field, d_ref_field, 256, d_out_cb, d_out_cr, out_pitch_bytes,
                      stream, true);
}

int hmme_predict_chroma_refs4_frame(hmme_ctx* ctx, const hmme_plane* const* refs, int n_refs, int width, int height, const hmme_frame_params* fp,
                                    const hmme_weight* wps, const int16_t* mv_field, const uint8_t* ref_field, void* const* outs, int out_stride) {
  if (!ctx) return HMME_ERR_ARG;
  return predict_refs_frame(ctx, "hmme_predict_chroma_refs4_frame", refs, n_refs, 2, width, height, fp, wps, mv_field, ref_field, 256, outs, out_stride, true);
}

// ---- L0, L1 or bi per PU: the decision over the four table sets of a B picture, and the prediction that follows it ---------------------------
int hmme_select_dirs_check(const hmme_select_params* sel, int n_pics, const hmme_dir_params* dirs) {
  char msg[256];
  return select_dirs_eval(sel, n_pics, dirs, msg, sizeof msg);
}

int hmme_select_dirs_device(hmme_ctx* ctx, int width, int height, int n_pics, const hmme_frame_params* fp, const hmme_select_params* sel,
                            const hmme_dir_params* dirs, const void* d_mv_uni, const void* d_cost_uni, const void* d_mv_bi, const void* d_cost_bi,
                            const void* d_uni_field, const void* d_pred_q, void* d_out_field, void* d_out_dir, void* d_out_slot, void* d_out_cost,
                            void* stream) {
  return select_device(ctx, SelectCall("hmme_select_dirs_device", kSelectDirs, width, height, n_pics, 1, fp, sel).with(dirs).with(kMv, d_mv_uni).with(kCost, d_cost_uni)
                           .with(kMvBi, d_mv_bi).with(kCostBi, d_cost_bi).with(kUniField, d_uni_field).with(kPredQ, d_pred_q).with(kOutField, d_out_field)
                           .with(kOutDir, d_out_dir).with(kOutSlot, d_out_slot).with(kOutCost, d_out_cost), (hipStream_t)stream);
}

int hmme_select_dirs_frame(hmme_ctx* ctx, int width, int height, const hmme_frame_params* fp, const hmme_select_params* sel,
                           const hmme_dir_params* dir, const int16_t* mv_uni, const uint32_t* cost_uni, const int16_t* mv_bi, const uint32_t* cost_bi,
                           const int16_t* uni_field, const int16_t* pred_q, int16_t* out_field, uint8_t* out_dir, uint16_t* out_slot,
                           uint32_t* out_cost) {
  return select_host(ctx, SelectCall("hmme_select_dirs_frame", kSelectDirs, width, height, 1, 1, fp, sel).with(dir).with(kMv, mv_uni).with(kCost, cost_uni)
                         .with(kMvBi, mv_bi).with(kCostBi, cost_bi).with(kUniField, uni_field).with(kPredQ, pred_q).with(kOutField, out_field)
                         .with(kOutDir, out_dir).with(kOutSlot, out_slot).with(kOutCost, out_cost));
}

// ... at one MV per 4x4 block: all 593 slots, with HM's isBipredRestriction (the rule: include/hmme.h)
int hmme_select_dirs4_check(const hmme_select_params* sel, int n_pics, const hmme_dir_params* dirs) {
  char msg[256];
  return select_dirs_eval(sel, n_pics, dirs, msg, sizeof msg, 256);
}

int hmme_select_dirs4_device(hmme_ctx* ctx, int width, int height, int n_pics, const hmme_frame_params* fp, const hmme_select_params* sel,
                             const hmme_dir_params* dirs, const void* d_mv_uni, const void* d_cost_uni, const void* d_mv_bi, const void* d_cost_bi,
                             const void* d_uni_field, const void* d_pred_q, void* d_out_field, void* d_out_dir, void* d_out_slot, void* d_out_cost,
                             void* stream) {
  if (!ctx) return HMME_ERR_ARG;
  return named(ctx, "hmme_select_dirs4_device", select_device(ctx, SelectCall("hmme_select_dirs4_device", kSelectDirs4, width, height, n_pics, 1, fp, sel).with(dirs).with(kMv, d_mv_uni).with(kCost, d_cost_uni)
                                .with(kMvBi, d_mv_bi).with(kCostBi, d_cost_bi).with(kUniField, d_uni_field).with(kPredQ, d_pred_q).with(kOutField, d_out_field)
                                .with(kOutDir, d_out_dir).with(kOutSlot, d_out_slot).with(kOutCost, d_out_cost), (hipStream_t)stream));   // the CTU range's refusal, too, names the entry
}

int hmme_select_dirs4_frame(hmme_ctx* ctx, int width, int height, const hmme_frame_params* fp, const hmme_select_params* sel,
                            const hmme_dir_params* dir, const int16_t* mv_uni, const uint32_t* cost_uni, const int16_t* mv_bi, const uint32_t* cost_bi,
                            const int16_t* uni_field, const int16_t* pred_q, int16_t* out_field, uint8_t* out_dir, uint16_t* out_slot,
                            uint32_t* out_cost) {
  if (!ctx) return HMME_ERR_ARG;
  return named(ctx, "hmme_select_dirs4_frame", select_host(ctx, SelectCall("hmme_select_dirs4_frame", kSelectDirs4, width, height, 1, 1, fp, sel).with(dir).with(kMv, mv_uni).with(kCost, cost_uni)
                              .with(kMvBi, mv_bi).with(kCostBi, cost_bi).with(kUniField, uni_field).with(kPredQ, pred_q).with(kOutField, out_field)
                              .with(kOutDir, out_dir).with(kOutSlot, out_slot).with(kOutCost, out_cost)));   // the CTU range's refusal, too, names the entry
}

// ---- L0, L1 or bi and the reference index per list, per PU: the decision over the table sets of a B picture with several references -----------
int hmme_select_dirs_refs_check(const hmme_select_params* sel, int n_pics, int n_refs_max, const hmme_dir_refs_params* dirs) {
  char msg[256];
  return select_dirs_refs_eval(sel, n_pics, n_refs_max, dirs, msg, sizeof msg);
}

int hmme_select_dirs_refs_device(hmme_ctx* ctx, int width, int height, int n_pics, int n_refs_max, const hmme_frame_params* fp, const hmme_select_params* sel,
                                 const hmme_dir_refs_params* dirs, const void* d_mv_uni, const void* d_cost_uni, const void* d_mv_bi, const void* d_cost_bi,
                                 const void* d_uni_field, const void* d_uni_ref, const void* d_pred_q, void* d_out_field, void* d_out_ref, void* d_out_dir,
                                 void* d_out_slot, void* d_out_cost, void* stream) {
  return select_device(ctx, SelectCall("hmme_select_dirs_refs_device", kSelectDirsRefs, width, height, n_pics, n_refs_max, fp, sel).with(dirs).with(kMv, d_mv_uni)
                           .with(kCost, d_cost_uni).with(kMvBi, d_mv_bi).with(kCostBi, d_cost_bi).with(kUniField, d_uni_field).with(kUniRef, d_uni_ref)
                           .with(kPredQ, d_pred_q).with(kOutField, d_out_field).with(kOutRef, d_out_ref).with(kOutDir, d_out_dir).with(kOutSlot, d_out_slot)
                           .with(kOutCost, d_out_cost), (hipStream_t)stream);
}

int hmme_select_dirs_refs_frame(hmme_ctx* ctx, int width, int height, int n_refs_max, const hmme_frame_params* fp, const hmme_select_params* sel,
                                const hmme_dir_refs_params* dir, const int16_t* mv_uni, const uint32_t* cost_uni, const int16_t* mv_bi, const uint32_t* cost_bi,
                                const int16_t* uni_field, const uint8_t* uni_ref, const int16_t* pred_q, int16_t* out_field, uint8_t* out_ref, uint8_t* out_dir,
                                uint16_t* out_slot, uint32_t* out_cost) {
  return select_host(ctx, SelectCall("hmme_select_dirs_refs_frame", kSelectDirsRefs, width, height, 1, n_refs_max, fp, sel).with(dir).with(kMv, mv_uni)
                         .with(kCost, cost_uni).with(kMvBi, mv_bi).with(kCostBi, cost_bi).with(kUniField, uni_field).with(kUniRef, uni_ref).with(kPredQ, pred_q)
                         .with(kOutField, out_field).with(kOutRef, out_ref).with(kOutDir, out_dir).with(kOutSlot, out_slot).with(kOutCost, out_cost));
}

// ... at one MV per 4x4 block: all 593 slots, with HM's isBipredRestriction (the rule: include/hmme.h, "B pictures with several references per
// list from one MV per 4x4 block"); every refusal names the entry, the CTU range's too
int hmme_select_dirs_refs4_check(const hmme_select_params* sel, int n_pics, int n_refs_max, const hmme_dir_refs_params* dirs) {
  char msg[256];
  return select_dirs_refs_eval(sel, n_pics, n_refs_max, dirs, msg, sizeof msg, 256);
}

int hmme_select_dirs_refs4_device(hmme_ctx* ctx, int width, int height, int n_pics, int n_refs_max, const hmme_frame_params* fp, const hmme_select_params* sel,
                                  const hmme_dir_refs_params* dirs, const void* d_mv_uni, const void* d_cost_uni, const void* d_mv_bi, const void* d_cost_bi,
                                  const void* d_uni_field, const void* d_uni_ref, const void* d_pred_q, void* d_out_field, void* d_out_ref, void* d_out_dir,
                                  void* d_out_slot, void* d_out_cost, void* stream) {
  if (!ctx) return HMME_ERR_ARG;
  return named(ctx, "hmme_select_dirs_refs4_device",
               select_device(ctx, SelectCall("hmme_select_dirs_refs4_device", kSelectDirsRefs4, width, height, n_pics, n_refs_max, fp, sel).with(dirs).with(kMv, d_mv_uni)
                                      .with(kCost, d_cost_uni).with(kMvBi, d_mv_bi).with(kCostBi, d_cost_bi).with(kUniField, d_uni_field).with(kUniRef, d_uni_ref)
                                      .with(kPredQ, d_pred_q).with(kOutField, d_out_field).with(kOutRef, d_out_ref).with(kOutDir, d_out_dir).with(kOutSlot, d_out_slot)
                                      .with(kOutCost, d_out_cost), (hipStream_t)stream));
}

int hmme_select_dirs_refs4_frame(hmme_ctx* ctx, int width, int height, int n_refs_max, const hmme_frame_params* fp, const hmme_select_params* sel,
                                 const hmme_dir_refs_params* dir, const int16_t* mv_uni, const uint32_t* cost_uni, const int16_t* mv_bi, const uint32_t* cost_bi,
                                 const int16_t* uni_field, const uint8_t* uni_ref, const int16_t* pred_q, int16_t* out_field, uint8_t* out_ref, uint8_t* out_dir,
                                 uint16_t* out_slot, uint32_t* out_cost) {
  if (!ctx) return HMME_ERR_ARG;
  return named(ctx, "hmme_select_dirs_refs4_frame",
               select_host(ctx, SelectCall("hmme_select_dirs_refs4_frame", kSelectDirsRefs4, width, height, 1, n_refs_max, fp, sel).with(dir).with(kMv, mv_uni)
                                    .with(kCost, cost_uni).with(kMvBi, mv_bi).with(kCostBi, cost_bi).with(kUniField, uni_field).with(kUniRef, uni_ref).with(kPredQ, pred_q)
                                    .with(kOutField, out_field).with(kOutRef, out_ref).with(kOutDir, out_dir).with(kOutSlot, out_slot).with(kOutCost, out_cost)));
}

namespace {
// every picture's two weights before anything is launched; the message names the picture
int check_predict_bi_weights(hmme_ctx* ctx, const char* who, const hmme_frame_params* fp, const hmme_weight* wps0, const hmme_weight* wps1, int n_pics, PredBiWp* bw) {
  if (!fp) return fail(ctx, HMME_ERR_ARG, "%s: null params", who);
  if (!wps0 || !wps1) return fail(ctx, HMME_ERR_ARG, "%s: null weights", who);
  char msg[256];
  for (int i = 0; i < n_pics; ++i) {
    const int rc = predict_bi_weight_eval(fp->bit_depth, &wps0[i], &wps1[i], bw ? &bw[i] : nullptr, msg, sizeof msg);
    if (rc) return fail(ctx, rc, "%s: picture %d: %s", who, i, msg);
  }
  return HMME_OK;
}

// hmme_predict_bi_device, _w_device and hmme_predict_chroma_bi_device: one launch per picture, every block from the planes its direction names.
// weighted: two weights per picture and component, each pair through predict_bi_weight_eval; WP = 0 for a picture without weights or with
// identities only, else 1.  Plane lists, weights and images hold `comps` entries per picture.
int predict_bi(hmme_ctx* ctx, const char* who, const hmme_plane* const* refs0, const hmme_plane* const* refs1, int n_pics, int comps, int width, int height,
               const hmme_frame_params* fp, const hmme_weight* wps0, const hmme_weight* wps1, bool weighted, const void* d_mv_field, const void* d_dir_field,
               int mv_per_ctu, void* const* d_outs, int out_pitch_bytes, void* stream, bool four = false) {
  const int per_pic = 2 * comps, max_pics = hmme::kMaxRefs / per_pic;
  if (!refs0 || !refs1 || n_pics < 1 || n_pics > max_pics) return fail(ctx, HMME_ERR_ARG, "%s: %d pictures outside 1..%d (or a null plane list)", who, n_pics, max_pics);
  PredBiWp bw[hmme::kMaxRefs / 2];   // entry comps * i + c: component c of picture i
  int rc = weighted ? check_predict_bi_weights(ctx, who, fp, wps0, wps1, comps * n_pics, bw) : HMME_OK;
  if (rc) return rc;
  const hmme_plane* planes[hmme::kMaxRefs];   // picture i: its list 0 planes, then its list 1 planes
  for (int i = 0; i < n_pics; ++i)
    for (int c = 0; c < comps; ++c) { planes[per_pic * i + c] = refs0[comps * i + c]; planes[per_pic * i + comps + c] = refs1[comps * i + c]; }
  PredictArgs a;
  rc = predict_args(ctx, who, planes, per_pic * n_pics, !d_dir_field || !d_outs, fp, nullptr, d_mv_field, mv_per_ctu, out_pitch_bytes, &a, comps == 2 ? "plane" : "picture", four);
  if (rc) return rc;
  for (int r = 0; r < comps * n_pics; ++r)
    if (!d_outs[r]) return fail(ctx, HMME_ERR_ARG, "%s: null output image", who);
  hipStream_t s = (hipStream_t)stream;
  PredictLaunch L;
  rc = predict_begin(ctx, who, planes, per_pic * n_pics, comps, width, height, fp, a, s, &L);
  if (rc || !L.acquired) return rc;
  const hmme_plane* p0 = planes[0];
  const size_t blocks = (size_t)L.n_ctu * mv_per_ctu;
  for (int i = 0; i < n_pics && rc == HMME_OK && L.count; ++i) {
    const int16_t* field = (const int16_t*)d_mv_field + blocks * 4 * i;
    const uint8_t* dirs = (const uint8_t*)d_dir_field + blocks * i;
    if (comps == 2) {
      hmme::MeChromaSrc src = {};
      for (int k = 0; k < 4; ++k) src.set.base[k] = planes[4 * i + k]->origin();
      src.field = dirs;
      src.n_ctu = L.n_ctu;
      if (bw[2 * i].identity && bw[2 * i + 1].identity)   // the 4x4 form is unweighted: always this one
        rc = launch_chroma<2, 0>(ctx, p0, src, field, mv_per_ctu, L, d_outs[2 * i], d_outs[2 * i + 1], out_pitch_bytes, s, hmme::MeChromaWp<2, 0>{});
      else
        rc = launch_chroma<2, 1>(ctx, p0, src, field, mv_per_ctu, L, d_outs[2 * i], d_outs[2 * i + 1], out_pitch_bytes, s, hmme::MeChromaWp<2, 1>{{bw[2 * i].k, bw[2 * i + 1].k}});
    } else {
      rc = launch_predict_bi(ctx, p0, planes[2 * i]->origin(), planes[2 * i + 1]->origin(), field, dirs, mv_per_ctu, L.first, L.count, (uint8_t*)d_outs[i], out_pitch_bytes, s,
                             bw[i].identity ? nullptr : &bw[i].k);
    }
    rc = named(ctx, who, rc);
  }
  return pairs_end(ctx, planes, planes, per_pic * n_pics, s, rc);   // whatever the launches returned: the scratch is acquired
}

// hmme_predict_bi_frame, _w_frame and hmme_predict_chroma_bi_frame; ref0 / ref1 / outs: `comps` entries each.  The weights answer first.
int predict_bi_frame(hmme_ctx* ctx, const char* who, const hmme_plane* const* ref0, const hmme_plane* const* ref1, int comps, int width, int height,
                     const hmme_frame_params* fp, const hmme_weight* wp0, const hmme_weight* wp1, bool weighted, const int16_t* mv_field, const uint8_t* dir_field,
                     int mv_per_ctu, void* const* outs, int out_stride, bool four = false) {
  int rc = weighted ? check_predict_bi_weights(ctx, who, fp, wp0, wp1, comps, nullptr) : HMME_OK;   // before anything is staged
  if (rc == HMME_OK) rc = bi_check(ctx, who, fp, 0);
  if (rc == HMME_OK) rc = frame_args(ctx, who, fp, ref0, comps, comps, !ref1 || !mv_field || !dir_field || frame_null_outs(outs, comps), mv_per_ctu, width, height, four);
  for (int c = 0; rc == HMME_OK && c < comps; ++c)
    if (!ref1[c]) rc = fail(ctx, HMME_ERR_ARG, "%s: null plane", who);
  if (rc) return rc;
  // blocks without a direction, too, come back as they were
  return frame_staged(ctx, who, ref0[0], comps, width, height, mv_field, dir_field, mv_per_ctu, outs, out_stride, 2, [&](void* d_field, void* d_dir_field, void* const* d_outs, int pitch, hipStream_t s) {
    return predict_bi(ctx, who, ref0, ref1, 1, comps, width, height, fp, wp0, wp1, weighted, d_field, d_dir_field, mv_per_ctu, d_outs, pitch, s, four);
  });
}
}  // namespace

int hmme_predict_bi_weight_check(int bit_depth, const hmme_weight* wp0, const hmme_weight* wp1) {
  char msg[256];
  return predict_bi_weight_eval(bit_depth, wp0, wp1, nullptr, msg, sizeof msg);
}

int hmme_predict_bi_device(hmme_ctx* ctx, const hmme_plane* const* refs0, const hmme_plane* const* refs1, int n_pics, const hmme_frame_params* fp,
                           const void* d_mv_field, const void* d_dir_field, int mv_per_ctu, void* const* d_outs, int out_pitch_bytes, void* stream) {
  if (!ctx) return HMME_ERR_ARG;
  return predict_bi(ctx, "hmme_predict_bi_device", refs0, refs1, n_pics, 1, 0, 0, fp, nullptr, nullptr, false, d_mv_field, d_dir_field, mv_per_ctu, d_outs,
                    out_pitch_bytes, stream);
}

int hmme_predict_bi_w_device(hmme_ctx* ctx, const hmme_plane* const* refs0, const hmme_plane* const* refs1, int n_pics, const hmme_frame_params* fp,
                             const hmme_weight* wps0, const hmme_weight* wps1, const void* d_mv_field, const void* d_dir_field, int mv_per_ctu,
                             void* const* d_outs, int out_pitch_bytes, void* stream) {
  if (!ctx) return HMME_ERR_ARG;
  return predict_bi(ctx, "hmme_predict_bi_w_device", refs0, refs1, n_pics, 1, 0, 0, fp, wps0, wps1, true, d_mv_field, d_dir_field, mv_per_ctu, d_outs, out_pitch_bytes,
                    stream);
}

int hmme_predict_bi_frame(hmme_ctx* ctx, const hmme_plane* ref0, const hmme_plane* ref1, const hmme_frame_params* fp, const int16_t* mv_field,
                          const uint8_t* dir_field, int mv_per_ctu, void* out, int out_stride) {
  if (!ctx) return HMME_ERR_ARG;
  return predict_bi_frame(ctx, "hmme_predict_bi_frame", &ref0, &ref1, 1, 0, 0, fp, nullptr, nullptr, false, mv_field, dir_field, mv_per_ctu, &out, out_stride);
}

int hmme_predict_bi_w_frame(hmme_ctx* ctx, const hmme_plane* ref0, const hmme_plane* ref1, const hmme_frame_params* fp, const hmme_weight* wp0,
                            const hmme_weight* wp1, const int16_t* mv_field, const uint8_t* dir_field, int mv_per_ctu, void* out, int out_stride) {
  if (!ctx) return HMME_ERR_ARG;
  return predict_bi_frame(ctx, "hmme_predict_bi_w_frame", &ref0, &ref1, 1, 0, 0, fp, wp0, wp1, true, mv_field, dir_field, mv_per_ctu, &out, out_stride);
}

// ---- the prediction of a B picture with several references per list (the rule: include/hmme.h) --------------------------------------------------
// ... from one MV and one direction per 4x4 block, unweighted, for Y and for the Cb / Cr of a 4:2:0 picture (me_predict_bi4_kernel,
// me_predict_chroma_bi4_kernel; the rule: include/hmme.h, "B pictures from one MV per 4x4 block")
int hmme_predict_bi4_device(hmme_ctx* ctx, const hmme_plane* const* refs0, const hmme_plane* const* refs1, int n_pics, const hmme_frame_params* fp,
                            const void* d_mv_field, const void* d_dir_field, void* const* d_outs, int out_pitch_bytes, void* stream) {
  if (!ctx) return HMME_ERR_ARG;
  return predict_bi(ctx, "hmme_predict_bi4_device", refs0, refs1, n_pics, 1, 0, 0, fp, nullptr, nullptr, false, d_mv_field, d_dir_field, 256, d_outs, out_pitch_bytes, stream,
                    true);
}

int hmme_predict_bi4_frame(hmme_ctx* ctx, const hmme_plane* ref0, const hmme_plane* ref1, const hmme_frame_params* fp, const int16_t* mv_field,
                           const uint8_t* dir_field, void* out, int out_stride) {
  if (!ctx) return HMME_ERR_ARG;
  return predict_bi_frame(ctx, "hmme_predict_bi4_frame", &ref0, &ref1, 1, 0, 0, fp, nullptr, nullptr, false, mv_field, dir_field, 256, &out, out_stride, true);
}

int hmme_predict_chroma_bi4_device(hmme_ctx* ctx, const hmme_plane* const* refs0, const hmme_plane* const* refs1, int n_pics, int width, int height,
                                   const hmme_frame_params* fp, const void* d_mv_field, const void* d_dir_field, void* const* d_outs, int out_pitch_bytes,
                                   void* stream) {
  if (!ctx) return HMME_ERR_ARG;
  return predict_bi(ctx, "hmme_predict_chroma_bi4_device", refs0, refs1, n_pics, 2, width, height, fp, nullptr, nullptr, false, d_mv_field, d_dir_field, 256, d_outs,
                    out_pitch_bytes, stream, true);
}

int hmme_predict_chroma_bi4_frame(hmme_ctx* ctx, const hmme_plane* const* ref0, const hmme_plane* const* ref1, int width, int height, const hmme_frame_params* fp,
                                  const int16_t* mv_field, const uint8_t* dir_field, void* const* outs, int out_stride) {
  if (!ctx) return HMME_ERR_ARG;
  return predict_bi_frame(ctx, "hmme_predict_chroma_bi4_frame", ref0, ref1, 2, width, height, fp, nullptr, nullptr, false, mv_field, dir_field, 256, outs, out_stride, true);
}

namespace {
// The weights of one component of such a picture as the kernels take them (hmme_predict_bi_refs_weight_check; the rule: include/hmme.h,
// "multi-reference B pictures: explicit weights and 4:2:0 chroma"): uni[l][r] is addWeightUni's form of list l's reference r, shift the
// slice's common shift' of addWeightBi.  The weight of list l's reference r is wps_l[stride * r] (stride 2: one component of (Cb, Cr) pairs).
struct PredBiRefsWp {
  bool identity = true;   // every weight of both lists: the picture is hmme_predict_bi_refs_device's
  hmme::MePredWp<1> uni[2][hmme::kMaxRefs] = {};
  int shift = 0;
};
// In the header's order: 1. the argument errors of every weight of list 0, then of list 1; 2. two unequal shifts; 3. each weight alone, list 0
// then list 1; 4. every pair (r0, r1), r0-major.  The message names the list and the reference(s).
int predict_bi_refs_weight_eval(int bit_depth, const hmme_weight* wps0, int n0, const hmme_weight* wps1, int n1, int stride, PredBiRefsWp* out, char* msg, size_t n) {
  const hmme_weight* const lists[2] = {wps0, wps1};
  const int cnt[2] = {n0, n1};
  static const char* const name[2] = {"L0", "L1"};
  char why[192];
  msg[0] = 0;
  for (int l = 0; l < 2; ++l) {
    if (bit_depth < 8 || bit_depth > 12) { snprintf(msg, n, "bit depth %d outside 8..12", bit_depth); return HMME_ERR_ARG; }
    if (!lists[l]) { snprintf(msg, n, "null weights of list %d", l); return HMME_ERR_ARG; }
    if (cnt[l] < 1 || cnt[l] > hmme::kMaxRefs) { snprintf(msg, n, "list %d: %d references outside 1..%d", l, cnt[l], hmme::kMaxRefs); return HMME_ERR_ARG; }
    for (int r = 0; r < cnt[l]; ++r) {
      const int rc = bi_weight_args(bit_depth, &lists[l][stride * r], name[l], why, sizeof why);
      if (rc) { snprintf(msg, n, "list %d reference %d: %s", l, r, why); return rc; }
    }
  }
  for (int l = 0; l < 2; ++l)
    for (int r = 0; r < cnt[l]; ++r)
      if (lists[l][stride * r].shift != wps0[0].shift) {
        snprintf(msg, n, "list %d reference %d: shift %d differs from list 0 reference 0's %d (one log2WeightDenom per slice and component)", l, r,
                 lists[l][stride * r].shift, wps0[0].shift);
        return HMME_ERR_ARG;
      }
  bool all = true;
  for (int l = 0; l < 2; ++l)
    for (int r = 0; r < cnt[l]; ++r) {
      bool id = true;
      hmme::MePredWp<1> pw;
      const int rc = other_weight_eval(bit_depth, &lists[l][stride * r], &id, &pw, why, sizeof why, name[l]);
      if (rc) { snprintf(msg, n, "list %d reference %d: %s", l, r, why); return rc; }
      all = all && id;
      if (out) out->uni[l][r] = pw;
    }
  for (int r0 = 0; r0 < n0; ++r0)
    for (int r1 = 0; r1 < n1; ++r1) {   // arguments and single lines have passed: only the pair's line can answer
      const int rc = predict_bi_weight_eval(bit_depth, &wps0[stride * r0], &wps1[stride * r1], nullptr, why, sizeof why);
      if (rc) { snprintf(msg, n, "list 0 reference %d with list 1 reference %d: %s", r0, r1, why); return rc; }
    }
  if (out) {
    out->identity = all;
    out->shift = wps0[0].shift + 1 + std::max(2, 14 - bit_depth);
  }
  return HMME_OK;
}

// the weights of a bi_refs prediction before anything else is looked at: comps == 2: (Cb, Cr) per reference, each component on its own
int check_predict_bi_refs_weights(hmme_ctx* ctx, const char* who, const hmme_frame_params* fp, const hmme_weight* wps0, int n0, const hmme_weight* wps1, int n1,
                                  int comps, PredBiRefsWp* bw) {
  if (!fp) return fail(ctx, HMME_ERR_ARG, "%s: null params", who);
  char msg[256];
  for (int c = 0; c < comps; ++c) {
    const int rc = predict_bi_refs_weight_eval(fp->bit_depth, wps0 ? wps0 + c : nullptr, n0, wps1 ? wps1 + c : nullptr, n1, comps, bw ? &bw[c] : nullptr, msg, sizeof msg);
    if (rc) return comps == 2 ? fail(ctx, rc, "%s: %s: %s", who, c ? "Cr" : "Cb", msg) : fail(ctx, rc, "%s: %s", who, msg);
  }
  return HMME_OK;
}
// what a list count may be: luma 1..16 planes per list (two plane sets), 4:2:0 2 * (n0 + n1) <= 16 planes in the ONE set of the chroma kernel
int bi_refs_counts(hmme_ctx* ctx, const char* who, const void* refs0, int n0, const void* refs1, int n1, int comps) {
  if (!refs0 || !refs1 || n0 < 1 || n0 > hmme::kMaxRefs || n1 < 1 || n1 > hmme::kMaxRefs)
    return fail(ctx, HMME_ERR_ARG, "%s: %d / %d reference pictures outside 1..%d (or a null plane list)", who, n0, n1, hmme::kMaxRefs);
  if (comps == 2 && 2 * (n0 + n1) > hmme::kMaxRefs)
    return fail(ctx, HMME_ERR_ARG, "%s: %d + %d reference pictures: a launch takes %d planes, %d references of both lists together", who, n0, n1, hmme::kMaxRefs, hmme::kMaxRefs / 2);
  return HMME_OK;
}

// hmme_predict_bi_refs_device, _w_device and hmme_predict_chroma_bi_refs_device: ONE picture, ONE launch, every block from the planes its
// direction and its two reference indices name.  Luma: me_predict_bi_kernel<T, 0 | 2, 1>, the two lists through the checks of predict_refs one
// after the other (each up to 16 planes), list 1 against list 0's first plane for the size.  4:2:0 (comps == 2; refs_l: (Cb, Cr) per reference):
// me_predict_chroma_kernel<T, 3, 0 | 2, PER> with list 0's planes, then list 1's, in one set.  weighted: the weights answer first; WP = 0
// without weights and where every weight is the identity, else every block goes through the weighted tails.
// four: hmme_predict_bi_refs4_device and hmme_predict_chroma_bi_refs4_device -- mv_per_ctu is 256, no weights; launch_predict_bi and
// launch_chroma then pick me_predict_bi4_kernel<T, 1> and me_predict_chroma_bi4_kernel<T, 1>.
int predict_bi_refs(hmme_ctx* ctx, const char* who, const hmme_plane* const* refs0, int n0, const hmme_plane* const* refs1, int n1, int comps, int width, int height,
                    const hmme_frame_params* fp, const hmme_weight* wps0, const hmme_weight* wps1, bool weighted, const void* d_mv_field, const void* d_dir_field,
                    const void* d_ref_field, int mv_per_ctu, void* d_out, void* d_out_cr, int out_pitch_bytes, void* stream, bool four = false) {
  PredBiRefsWp bw[2];
  int rc = weighted ? check_predict_bi_refs_weights(ctx, who, fp, wps0, n0, wps1, n1, comps, bw) : HMME_OK;
  if (rc == HMME_OK) rc = bi_check(ctx, who, fp, 0);
  if (rc == HMME_OK) rc = bi_refs_counts(ctx, who, refs0, n0, refs1, n1, comps);
  if (rc) return rc;
  const bool null_arg = !d_dir_field || !d_ref_field || !d_out || (comps == 2 && !d_out_cr);
  hipStream_t s = (hipStream_t)stream;
  PredictArgs a;
  PredictLaunch L;
  if (comps == 2) {
    const int np = 2 * (n0 + n1);
    const hmme_plane* planes[hmme::kMaxRefs];   // list 0's (Cb, Cr) pairs, then list 1's: the kernel's set
    for (int r = 0; r < 2 * n0; ++r) planes[r] = refs0[r];
    for (int r = 0; r < 2 * n1; ++r) planes[2 * n0 + r] = refs1[r];
    rc = predict_args(ctx, who, planes, np, null_arg, fp, nullptr, d_mv_field, mv_per_ctu, out_pitch_bytes, &a, "plane", four);
    if (rc) return rc;
    rc = predict_begin(ctx, who, planes, np, 2, width, height, fp, a, s, &L);
    if (rc || !L.acquired) return rc;
    if (L.count) {
      const hmme::MeChromaSrc src = {L.pl.refs, (const uint8_t*)d_dir_field, n0, L.n_ctu};
      if (weighted && !(bw[0].identity && bw[1].identity)) {
        hmme::MeChromaWp<3, 2> cw = {};
        cw.ref_field = (const uint8_t*)d_ref_field; cw.n_refs1 = n1;
        for (int c = 0; c < 2; ++c) {
          cw.shift[c] = bw[c].shift;
          for (int r = 0; r < n0; ++r) cw.ref[2 * r + c] = bw[c].uni[0][r];
          for (int r = 0; r < n1; ++r) cw.ref[2 * (n0 + r) + c] = bw[c].uni[1][r];
        }
        rc = launch_chroma<3, 2>(ctx, planes[0], src, (const int16_t*)d_mv_field, mv_per_ctu, L, d_out, d_out_cr, out_pitch_bytes, s, cw);
      } else {
        rc = launch_chroma<3, 0>(ctx, planes[0], src, (const int16_t*)d_mv_field, mv_per_ctu, L, d_out, d_out_cr, out_pitch_bytes, s,
                                 hmme::MeChromaWp<3, 0>{(const uint8_t*)d_ref_field, n1});
      }
    }
    return pairs_end(ctx, planes, planes, np, s, rc);   // whatever the launch returned: the scratch is acquired
  }
  rc = predict_args(ctx, who, refs0, n0, null_arg, fp, nullptr, d_mv_field, mv_per_ctu, out_pitch_bytes, &a, "reference", four);
  if (rc) return rc;
  const hmme_plane* first0[hmme::kMaxRefs];
  for (int r = 0; r < n1; ++r) {
    if (!refs1[r]) return fail(ctx, HMME_ERR_ARG, "%s: null plane", who);
    first0[r] = refs0[0];
  }
  rc = predict_begin(ctx, who, refs0, n0, 1, 0, 0, fp, a, s, &L);
  PairLaunch l1;   // list 1: this context, fp's bit depth, list 0's size; ordered like references
  if (rc == HMME_OK) rc = named(ctx, who, pairs_begin(ctx, first0, refs1, n1, &a.f, s, &l1));
  if (rc || !L.acquired) return rc;
  const hmme_plane* p0 = refs0[0];
  const hmme::MePredBiRefs<1> br = {{L.pl.refs, l1.refs}, (const uint8_t*)d_ref_field, {n0, n1}};
  hmme::MePredBiWp<2> kw = {};
  const bool wp = weighted && !bw[0].identity;
  if (wp) {
    for (int l = 0; l < 2; ++l)
      for (int r = 0; r < (l ? n1 : n0); ++r) kw.ref[l][r] = bw[0].uni[l][r];
    kw.shift = bw[0].shift;
  }
  rc = named(ctx, who, launch_predict_bi(ctx, p0, nullptr, nullptr, (const int16_t*)d_mv_field, (const uint8_t*)d_dir_field, mv_per_ctu, L.first, L.count, (uint8_t*)d_out,
                                         out_pitch_bytes, s, nullptr, &br, wp ? &kw : nullptr));
  return lists_end(ctx, refs0, n0, refs1, n1, s, rc);   // whatever the launch returned: the scratch is acquired
}

// the _frame forms of the three; refs_l: `comps` planes per reference, outs: `comps` images.  The weights answer first.
int predict_bi_refs_frame(hmme_ctx* ctx, const char* who, const hmme_plane* const* refs0, int n0, const hmme_plane* const* refs1, int n1, int comps, int width, int height,
                          const hmme_frame_params* fp, const hmme_weight* wps0, const hmme_weight* wps1, bool weighted, const int16_t* mv_field, const uint8_t* dir_field,
                          const uint8_t* ref_field, int mv_per_ctu, void* const* outs, int out_stride, bool four = false) {
  int rc = weighted ? check_predict_bi_refs_weights(ctx, who, fp, wps0, n0, wps1, n1, comps, nullptr) : HMME_OK;   // before anything is staged
  if (rc == HMME_OK) rc = bi_check(ctx, who, fp, 0);
  if (rc) return rc;
  if (comps == 2) rc = bi_refs_counts(ctx, who, refs0, n0, refs1, n1, comps);
  else if (!refs0 || !refs1 || n0 < 1 || n0 > hmme::kMaxRefs || n1 < 1 || n1 > hmme::kMaxRefs || !refs0[0])
    rc = fail(ctx, HMME_ERR_ARG, "%s: %d / %d reference pictures outside 1..%d (or a null plane)", who, n0, n1, hmme::kMaxRefs);
  if (rc) return rc;
  if (comps == 2 && !refs0[0]) return fail(ctx, HMME_ERR_ARG, "%s: null plane", who);
  rc = frame_args(ctx, who, fp, refs0, comps * n0, comps, !mv_field || !dir_field || !ref_field || frame_null_outs(outs, comps), mv_per_ctu, width, height, four);
  if (rc == HMME_OK) rc = frame_args(ctx, who, fp, refs1, comps * n1, comps, false, mv_per_ctu, width, height, four);
  if (rc) return rc;
  const hmme_plane* p0 = refs0[0];
  if (p0->ctx != ctx) return fail(ctx, HMME_ERR_ARG, "%s: plane belongs to another context (planes are used with the context that created them)", who);
  if (out_stride < p0->width) return fail(ctx, HMME_ERR_ARG, "%s: output stride %d below the picture width", who, out_stride);
  // blocks without a direction or a reference, too, come back as they were
  const size_t blocks = (size_t)(comps == 2 ? hmme_num_ctus(width, height) : p0->n_ctu) * mv_per_ctu, row = (size_t)p0->width * p0->bps;
  Stage st(ctx);
  const int field = st.in(mv_field, sizeof(int16_t) * 2 * blocks * 2), dirs = st.in(dir_field, blocks), rfield = st.in(ref_field, 2 * blocks);
  const int img = st.image(outs[0], row, p0->height, (size_t)out_stride * p0->bps);
  const int img1 = st.image(comps == 2 ? outs[1] : nullptr, row, p0->height, (size_t)out_stride * p0->bps);
  rc = st.begin();
  if (rc == HMME_OK)
    rc = predict_bi_refs(ctx, who, refs0, n0, refs1, n1, comps, width, height, fp, wps0, wps1, weighted, st.at(field), st.at(dirs), st.at(rfield), mv_per_ctu, st.at(img),
                         st.at(img1), (int)row, ctx->stream, four);
  return rc ? rc : st.end();
}
}  // namespace

int hmme_predict_bi_refs_device(hmme_ctx* ctx, const hmme_plane* const* refs0, int n0, const hmme_plane* const* refs1, int n1, const hmme_frame_params* fp,
                                const void* d_mv_field, const void* d_dir_field, const void* d_ref_field, int mv_per_ctu, void* d_out, int out_pitch_bytes,
                                void* stream) {
  if (!ctx) return HMME_ERR_ARG;
  return predict_bi_refs(ctx, "hmme_predict_bi_refs_device", refs0, n0, refs1, n1, 1, 0, 0, fp, nullptr, nullptr, false, d_mv_field, d_dir_field, d_ref_field, mv_per_ctu,
                         d_out, nullptr, out_pitch_bytes, stream);
}

int hmme_predict_bi_refs_frame(hmme_ctx* ctx, const hmme_plane* const* refs0, int n0, const hmme_plane* const* refs1, int n1, const hmme_frame_params* fp,
                               const int16_t* mv_field, const uint8_t* dir_field, const uint8_t* ref_field, int mv_per_ctu, void* out, int out_stride) {
  if (!ctx) return HMME_ERR_ARG;
  return predict_bi_refs_frame(ctx, "hmme_predict_bi_refs_frame", refs0, n0, refs1, n1, 1, 0, 0, fp, nullptr, nullptr, false, mv_field, dir_field, ref_field, mv_per_ctu,
                               &out, out_stride);
}

// ---- ... with a weight per reference, and for Cb / Cr (the rule: include/hmme.h, "multi-reference B pictures: explicit weights and 4:2:0 chroma")
int hmme_predict_bi_refs_weight_check(int bit_depth, const hmme_weight* wps0, int n0, const hmme_weight* wps1, int n1) {
  char msg[256];
  return predict_bi_refs_weight_eval(bit_depth, wps0, n0, wps1, n1, 1, nullptr, msg, sizeof msg);
}

int hmme_predict_bi_refs_w_device(hmme_ctx* ctx, const hmme_plane* const* refs0, int n0, const hmme_plane* const* refs1, int n1, const hmme_frame_params* fp,
                                  const hmme_weight* wps0, const hmme_weight* wps1, const void* d_mv_field, const void* d_dir_field, const void* d_ref_field,
                                  int mv_per_ctu, void* d_out, int out_pitch_bytes, void* stream) {
  if (!ctx) return HMME_ERR_ARG;
  return predict_bi_refs(ctx, "hmme_predict_bi_refs_w_device", refs0, n0, refs1, n1, 1, 0, 0, fp, wps0, wps1, true, d_mv_field, d_dir_field, d_ref_field, mv_per_ctu, d_out,
                         nullptr, out_pitch_bytes, stream);
}

int hmme_predict_bi_refs_w_frame(hmme_ctx* ctx, const hmme_plane* const* refs0, int n0, const hmme_plane* const* refs1, int n1, const hmme_frame_params* fp,
                                 const hmme_weight* wps0, const hmme_weight* wps1, const int16_t* mv_field, const uint8_t* dir_field, const uint8_t* ref_field,
                                 int mv_per_ctu, void* out, int out_stride) {
  if (!ctx) return HMME_ERR_ARG;
  return predict_bi_refs_frame(ctx, "hmme_predict_bi_refs_w_frame", refs0, n0, refs1, n1, 1, 0, 0, fp, wps0, wps1, true, mv_field, dir_field, ref_field, mv_per_ctu, &out,
                               out_stride);
}

int hmme_predict_chroma_bi_refs_device(hmme_ctx* ctx, const hmme_plane* const* refs0, int n0, const hmme_plane* const* refs1, int n1, int width, int height,
                                       const hmme_frame_params* fp, const hmme_weight* wps0, const hmme_weight* wps1, const void* d_mv_field, const void* d_dir_field,
                                       const void* d_ref_field, int mv_per_ctu, void* d_out_cb, void* d_out_cr, int out_pitch_bytes, void* stream) {
  if (!ctx) return HMME_ERR_ARG;
  return predict_bi_refs(ctx, "hmme_predict_chroma_bi_refs_device", refs0, n0, refs1, n1, 2, width, height, fp, wps0, wps1, wps0 || wps1, d_mv_field, d_dir_field, d_ref_field,
                         mv_per_ctu, d_out_cb, d_out_cr, out_pitch_bytes, stream);
}

int hmme_predict_chroma_bi_refs_frame(hmme_ctx* ctx, const hmme_plane* const* refs0, int n0, const hmme_plane* const* refs1, int n1, int width, int height,
                                      const hmme_frame_params* fp, const hmme_weight* wps0, const hmme_weight* wps1, const int16_t* mv_field, const uint8_t* dir_field,
                                      const uint8_t* ref_field, int mv_per_ctu, void* const* outs, int out_stride) {
  if (!ctx) return HMME_ERR_ARG;
  return predict_bi_refs_frame(ctx, "hmme_predict_chroma_bi_refs_frame", refs0, n0, refs1, n1, 2, width, height, fp, wps0, wps1, wps0 || wps1, mv_field, dir_field, ref_field,
                               mv_per_ctu, outs, out_stride);
}

// ... from one (direction, MV0, MV1, ref0, ref1) per 4x4 block, unweighted, for Y and for the Cb / Cr of a 4:2:0 picture (me_predict_bi4_kernel<T, 1>,
// me_predict_chroma_bi4_kernel<T, 1>; the rule: include/hmme.h, "B pictures with several references per list from one MV per 4x4 block")
int hmme_predict_bi_refs4_device(hmme_ctx* ctx, const hmme_plane* const* refs0, int n0, const hmme_plane* const* refs1, int n1, const hmme_frame_params* fp,
                                 const void* d_mv_field, const void* d_dir_field, const void* d_ref_field, void* d_out, int out_pitch_bytes, void* stream) {
  if (!ctx) return HMME_ERR_ARG;
  return named(ctx, "hmme_predict_bi_refs4_device", predict_bi_refs(ctx, "hmme_predict_bi_refs4_device", refs0, n0, refs1, n1, 1, 0, 0, fp, nullptr, nullptr, false, d_mv_field,
                                                                    d_dir_field, d_ref_field, 256, d_out, nullptr, out_pitch_bytes, stream, true));
}

int hmme_predict_bi_refs4_frame(hmme_ctx* ctx, const hmme_plane* const* refs0, int n0, const hmme_plane* const* refs1, int n1, const hmme_frame_params* fp,
                                const int16_t* mv_field, const uint8_t* dir_field, const uint8_t* ref_field, void* out, int out_stride) {
  if (!ctx) return HMME_ERR_ARG;
  return named(ctx, "hmme_predict_bi_refs4_frame", predict_bi_refs_frame(ctx, "hmme_predict_bi_refs4_frame", refs0, n0, refs1, n1, 1, 0, 0, fp, nullptr, nullptr, false, mv_field,
                                                                         dir_field, ref_field, 256, &out, out_stride, true));
}

int hmme_predict_chroma_bi_refs4_device(hmme_ctx* ctx, const hmme_plane* const* refs0, int n0, const hmme_plane* const* refs1, int n1, int width, int height,
                                        const hmme_frame_params* fp, const void* d_mv_field, const void* d_dir_field, const void* d_ref_field, void* d_out_cb,
                                        void* d_out_cr, int out_pitch_bytes, void* stream) {
  if (!ctx) return HMME_ERR_ARG;
  return named(ctx, "hmme_predict_chroma_bi_refs4_device", predict_bi_refs(ctx, "hmme_predict_chroma_bi_refs4_device", refs0, n0, refs1, n1, 2, width, height, fp, nullptr, nullptr,
                                                                           false, d_mv_field, d_dir_field, d_ref_field, 256, d_out_cb, d_out_cr, out_pitch_bytes, stream, true));
}

int hmme_predict_chroma_bi_refs4_frame(hmme_ctx* ctx, const hmme_plane* const* refs0, int n0, const hmme_plane* const* refs1, int n1, int width, int height,
                                       const hmme_frame_params* fp, const int16_t* mv_field, const uint8_t* dir_field, const uint8_t* ref_field, void* const* outs,
                                       int out_stride) {
  if (!ctx) return HMME_ERR_ARG;
  return named(ctx, "hmme_predict_chroma_bi_refs4_frame", predict_bi_refs_frame(ctx, "hmme_predict_chroma_bi_refs4_frame", refs0, n0, refs1, n1, 2, width, height, fp, nullptr,
                                                                                nullptr, false, mv_field, dir_field, ref_field, 256, outs, out_stride, true));
}

// ---- 4:2:0 chroma motion compensation from the luma motion fields ------------------------------------------------------------------------------
// The three prediction forms for Cb and Cr (me_predict_chroma_kernel; the rule: include/hmme.h): the bodies of the luma forms with two
// components (predict_begin).
int hmme_predict_chroma_pairs_device(hmme_ctx* ctx, const hmme_plane* const* refs, int n_pairs, int width, int height, const hmme_frame_params* fp,
                                     const hmme_weight* wps, const void* d_mv_field, int mv_per_ctu, void* const* d_outs, int out_pitch_bytes, void* stream) {
  if (!ctx) return HMME_ERR_ARG;
  return predict_pairs(ctx, "hmme_predict_chroma_pairs_device", refs, n_pairs, 2, width, height, fp, wps, d_mv_field, mv_per_ctu, d_outs, out_pitch_bytes, stream);
}

int hmme_predict_chroma_frame(hmme_ctx* ctx, const hmme_plane* const* ref, int width, int height, const hmme_frame_params* fp, const hmme_weight* wp,
                              const int16_t* mv_field, int mv_per_ctu, void* const* outs, int out_stride) {
  if (!ctx) return HMME_ERR_ARG;
  return predict_frame(ctx, "hmme_predict_chroma_frame", ref, 2, width, height, fp, wp, mv_field, mv_per_ctu, outs, out_stride);
}

int hmme_predict_chroma_refs_device(hmme_ctx* ctx, const hmme_plane* const* refs, int n_refs, int width, int height, const hmme_frame_params* fp,
                                    const hmme_weight* wps, const void* d_mv_field, const void* d_ref_field, int mv_per_ctu, void* d_out_cb, void* d_out_cr,
                                    int out_pitch_bytes, void* stream) {
  if (!ctx) return HMME_ERR_ARG;
  return predict_refs(ctx, "hmme_predict_chroma_refs_device", refs, n_refs, 2, width, height, fp, wps, d_mv_field, d_ref_field, mv_per_ctu, d_out_cb, d_out_cr,
                      out_pitch_bytes, stream);
}

int hmme_predict_chroma_refs_frame(hmme_ctx* ctx, const hmme_plane* const* refs, int n_refs, int width, int height, const hmme_frame_params* fp,
                                   const hmme_weight* wps, const int16_t* mv_field, const uint8_t* ref_field, int mv_per_ctu, void* const* outs, int out_stride) {
  if (!ctx) return HMME_ERR_ARG;
  return predict_refs_frame(ctx, "hmme_predict_chroma_refs_frame", refs, n_refs, 2, width, height, fp, wps, mv_field, ref_field, mv_per_ctu, outs, out_stride);
}

int hmme_predict_chroma_bi_device(hmme_ctx* ctx, const hmme_plane* const* refs0, const hmme_plane* const* refs1, int n_pics, int width, int height,
                                  const hmme_frame_params* fp, const hmme_weight* wps0, const hmme_weight* wps1, const void* d_mv_field, const void* d_dir_field,
                                  int mv_per_ctu, void* const* d_outs, int out_pitch_bytes, void* stream) {
  if (!ctx) return HMME_ERR_ARG;
  return predict_bi(ctx, "hmme_predict_chroma_bi_device", refs0, refs1, n_pics, 2, width, height, fp, wps0, wps1, wps0 || wps1, d_mv_field, d_dir_field, mv_per_ctu,
                    d_outs, out_pitch_bytes, stream);
}

int hmme_predict_chroma_bi_frame(hmme_ctx* ctx, const hmme_plane* const* ref0, const hmme_plane* const* ref1, int width, int height, const hmme_frame_params* fp,
                                 const hmme_weight* wp0, const hmme_weight* wp1, const int16_t* mv_field, const uint8_t* dir_field, int mv_per_ctu, void* const* outs,
                                 int out_stride) {
  if (!ctx) return HMME_ERR_ARG;
  return predict_bi_frame(ctx, "hmme_predict_chroma_bi_frame", ref0, ref1, 2, width, height, fp, wp0, wp1, wp0 || wp1, mv_field, dir_field, mv_per_ctu, outs, out_stride);
}

// ---- estimating explicit weighted-prediction parameters ----------------------------------------------------------------------------------------
// WeightPredAnalysis::xCalcACDCParamSlice / xEstimateWPParamSlice / xUpdatingWPParameters / xSelectWP / xCalcSADvalueWP
// (WeightPredAnalysis.cpp:67-120, :172-351) for luma alone and for the three components of a 4:2:0 slice: the whole-picture sums are kernels
// (me_plane_set_stats_kernel -- for a set of one plane its entry me_plane_stats_kernel -- and me_wp_sad_set_kernel: the 1 + n planes and n
// pairs of a luma call, the 3 (1 + n) and 3 n of a 4:2:0 call),
// the scalar derivation between and behind them is two pure functions in HM's own double / Int64 arithmetic (wp_parameters, wp_select).
// Synchronous, on the context's private stream.
namespace {
// kWpEst: [2 i] / [2 i + 1] = sample sum and AC of plane i of the call, then two sums per (reference, component) of the SAD pass
constexpr int kWpSetSad = 2 * hmme::kMaxSetPlanes;
constexpr int kWpSetWords = kWpSetSad + 2 * hmme::kMaxSetPairs;
constexpr int kWpStatBlocks = 1024;   // workgroups of one launch at most: each ends in one atomic add per sum

// lanes per row (log2) and workgroups of a reduction over the picture area of `pl`, n_y of them side by side (me_kernels.hpp: the geometry
// shared by the two kernels); rows are dealt evenly over the rounds a capped grid needs
struct StatGrid { int lpr_log2; unsigned blocks; };
StatGrid stat_grid(const hmme_plane* pl, int n_y) {
  const int nvec = (pl->width * pl->bps + 15) / 16;
  int l = 0;
  while ((1 << l) < nvec && l < 8) ++l;
  const int rpb = 256 >> l, row_blocks = (pl->height + rpb - 1) / rpb, cap = std::max(1, kWpStatBlocks / n_y);
  const int rounds = (row_blocks + cap - 1) / cap;
  return {l, (unsigned)((row_blocks + rounds - 1) / rounds)};
}

// one table entry per plane, the grid's x extent that of the plane that needs most workgroups
hmme::MePlaneDesc plane_desc(const hmme_plane* pl, int n_y, unsigned* blocks) {
  const StatGrid g = stat_grid(pl, n_y);
  *blocks = std::max(*blocks, g.blocks);
  return {pl->origin(), pl->pitch, pl->width, pl->height, g.lpr_log2};
}
// the two passes of xCalcACDCParamSlice over n (1..kMaxSetPlanes) planes of one sample type in two launches: sums[2 i], sums[2 i + 1] (zero on
// entry); pass 1 reads what pass 0 left, same stream.  A set of one plane goes without the table (me_plane_stats_kernel: the same body)
int launch_stats_set(hmme_ctx* ctx, const hmme_plane* const* pl, int n, unsigned long long* sums, hipStream_t s) {
  hmme::MePlaneSet set = {};
  unsigned blocks = 1;
  for (int i = 0; i < n; ++i) set.p[i] = plane_desc(pl[i], n, &blocks);
  auto passes = [&](auto one0, auto one1, auto set0, auto set1) {
    if (n == 1) {
      hipLaunchKernelGGL(one0, dim3(blocks), dim3(256), 0, s, set.p[0], sums);
      hipLaunchKernelGGL(one1, dim3(blocks), dim3(256), 0, s, set.p[0], sums);
    } else {
      hipLaunchKernelGGL(set0, dim3(blocks, (unsigned)n), dim3(256), 0, s, set, sums);
      hipLaunchKernelGGL(set1, dim3(blocks, (unsigned)n), dim3(256), 0, s, set, sums);
    }
  };
  if (pl[0]->bps == 1)
    passes(hmme::me_plane_stats_kernel<uint8_t, 0>, hmme::me_plane_stats_kernel<uint8_t, 1>, hmme::me_plane_set_stats_kernel<uint8_t, 0>, hmme::me_plane_set_stats_kernel<uint8_t, 1>);
  else
    passes(hmme::me_plane_stats_kernel<uint16_t, 0>, hmme::me_plane_stats_kernel<uint16_t, 1>, hmme::me_plane_set_stats_kernel<uint16_t, 0>, hmme::me_plane_set_stats_kernel<uint16_t, 1>);
  HIP_TRY(ctx, hipGetLastError());
  return HMME_OK;
}
// xCalcSADvalueWP of the comps (1 or 3) components of `cur` against those of n_refs references in one launch: pair comps r + c =
// refs[comps r + c] against cur[c], a.weight / offset / log2_denom filled in by the caller; two sums per pair (zero on entry)
int launch_wp_sad_set(hmme_ctx* ctx, const hmme_plane* const* cur, const hmme_plane* const* refs, int comps, int n_refs, hmme::MeWpSadSet& a,
                      unsigned long long* sums, hipStream_t s) {
  const int n_pairs = comps * n_refs;
  unsigned blocks = 1;
  a.comps = comps;
  for (int c = 0; c < comps; ++c) a.cur[c] = plane_desc(cur[c], n_pairs, &blocks);
  for (int i = 0; i < n_pairs; ++i) a.ref[i] = refs[i]->origin();
  const dim3 grid(blocks, (unsigned)n_pairs);
  if (cur[0]->bps == 1) hipLaunchKernelGGL(hmme::me_wp_sad_set_kernel<uint8_t>, grid, dim3(256), 0, s, a, sums);
  else hipLaunchKernelGGL(hmme::me_wp_sad_set_kernel<uint16_t>, grid, dim3(256), 0, s, a, sums);
  HIP_TRY(ctx, hipGetLastError());
  return HMME_OK;
}

// kernels on `s` read planes[0 .. n): what pairs_begin / pairs_end do for the planes of picture pairs -- the scratch (kWpEst) and the last fill of
// every plane before, one event of the context's ring behind, so that a refill of any of them on another stream waits
int planes_read_begin(hmme_ctx* ctx, const hmme_plane* const* planes, int n, hipStream_t s) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc = ensure(ctx, ctx->buf[kWpEst], sizeof(unsigned long long) * kWpSetWords);
  if (rc == HMME_OK) rc = scratch_acquire(ctx, s);
  for (int i = 0; i < n && rc == HMME_OK; ++i) rc = plane_wait(ctx, planes[i], s);
  return rc;
}
int planes_read_end(hmme_ctx* ctx, const hmme_plane* const* planes, int n, hipStream_t s, int rc) {
  for (int i = 0; i < n; ++i) {
    const int r2 = plane_read_chain(ctx, planes[i], s);
    if (rc == HMME_OK) rc = r2;
  }
  const int r3 = launch_end(ctx, s);
  if (r3 == HMME_OK)
    for (int i = 0; i < n; ++i) plane_read_mark(ctx, planes[i], s);
  return rc ? rc : r3;
}

// the sums of every plane of the list (of one sample type, up to kMaxSetPlanes) that has none cached: two launches for all of them, one
// download, one wait
int collect_stats(hmme_ctx* ctx, const hmme_plane* const* planes, int n, hipStream_t s) {
  const hmme_plane* todo[hmme::kMaxSetPlanes];
  int n_todo = 0;
  for (int i = 0; i < n; ++i) {
    if (planes[i]->stats_valid) continue;
    int q = 0;
    while (q < n_todo && todo[q] != planes[i]) ++q;
    if (q == n_todo) todo[n_todo++] = planes[i];
  }
  if (n_todo == 0) return HMME_OK;
  int rc = planes_read_begin(ctx, todo, n_todo, s);
  if (rc) return rc;
  unsigned long long h[2 * hmme::kMaxSetPlanes];
  unsigned long long* d_sums = ctx->buf[kWpEst].as<unsigned long long>();
  hipError_t e = hipMemsetAsync(d_sums, 0, sizeof(unsigned long long) * 2 * n_todo, s);
  if (e != hipSuccess) rc = fail(ctx, HMME_ERR_DEVICE, "plane statistics: %s", hipGetErrorString(e));
  if (rc == HMME_OK) rc = launch_stats_set(ctx, todo, n_todo, d_sums, s);
  if (rc == HMME_OK && (e = hipMemcpyAsync(h, d_sums, sizeof(unsigned long long) * 2 * n_todo, hipMemcpyDeviceToHost, s)) != hipSuccess)
    rc = fail(ctx, HMME_ERR_DEVICE, "plane statistics: %s", hipGetErrorString(e));
  rc = planes_read_end(ctx, todo, n_todo, s, rc);
  if (rc) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(s));
  for (int j = 0; j < n_todo; ++j) {
    todo[j]->stats_dc = (int64_t)h[2 * j]; todo[j]->stats_ac = (int64_t)h[2 * j + 1];
    todo[j]->stats_valid = true;
  }
  return HMME_OK;
}

// The estimator's arithmetic: pure functions, no context, no device (hmme_test_wp_parameters / hmme_test_wp_select show them to the CPU tests).
// comps = 1 (luma alone) or 3 (Y, Cb, Cr of a 4:2:0 slice); plane i of a call is component i % comps of the current picture (i < comps) or of
// reference i / comps - 1; stats[2 i], stats[2 i + 1] = its (dc_sum, ac), n_samples[c] = the sample count of component c; entry comps r + c
// belongs to component c of reference r.

// xEstimateWPParamSlice (:172-196): xUpdatingWPParameters (:200-268) from log2_denom_start (3..7) downwards until every weight is in range --
// reference outer, component inner, the first weight out of range ends a pass.  -> *log2_denom and (weight, clipped offset) of every entry
void wp_parameters(const int64_t* stats, const int64_t* n_samples, int comps, int n_refs, int bd, int log2_denom_start, int* log2_denom, int* weight,
                   int* offset) {
  auto norm_dc = [&](int plane) { const int64_t n = n_samples[plane % comps]; return (stats[2 * plane] + (n >> 1)) / n; };   // :115 without the RExt precision shift
  int d = log2_denom_start;
  for (;; --d) {   // ends at d = 3 at the latest: dWeight <= 15 puts weight in [0, 120], (1 << 3) - weight in [-112, 8]
    const int real_d = d + (bd - 8);
    bool in_range = true;
    for (int i = 0; i < comps * n_refs && in_range; ++i) {
      const int c = i % comps;
      const int64_t cur_dc = norm_dc(c), cur_ac = stats[2 * c + 1], ref_dc = norm_dc(comps + i), ref_ac = stats[2 * (comps + i) + 1];
      const double dw = ref_ac == 0 ? 1.0 : std::min(std::max(-16.0, (double)cur_ac / (double)ref_ac), 15.0);        // :234
      const int wgt = (int)(0.5 + dw * (double)(1 << d));                                                             // :235
      const int off = (int)(((cur_dc << d) - (int64_t)wgt * ref_dc + ((int64_t)1 << (real_d - 1))) >> real_d);        // :236
      weight[i] = wgt;
      if (c) {                                                                                                         // :239-245, range = 128
        const int pred = 128 - ((128 * wgt) >> d);
        const int delta_off = std::min(std::max(-512, off - pred), 511);
        offset[i] = std::min(std::max(-128, delta_off + pred), 127);
      } else {
        offset[i] = std::min(std::max(-128, off), 127);                                                                // :248
      }
      const int delta = (1 << d) - wgt;                                                                                // :252-258
      in_range = !(delta >= 128 || delta < -128);
    }
    if (in_range) break;
  }
  *log2_denom = d;
}

// xSelectWP (:272-320) on what wp_parameters gave and the two raw sums per entry as me_wp_sad_set_kernel leaves them (sums[2 i] weighted,
// sums[2 i + 1] unweighted before its << d), then TComSlice::initWpScaling (TComSlice.cpp:1487-1512: what the search, the refinement and the
// prediction take) -> wp[i] and, where given, info[i] of every entry
void wp_select(const int64_t* stats, const int64_t* n_samples, int comps, int n_refs, int bd, int d, const int* weight, const int* offset,
               const unsigned long long* sums, hmme_weight* wp, hmme_wp_info* info) {
  for (int r = 0; r < n_refs; ++r) {
    int64_t sad_wp[3], sad_nowp[3], sum_wp = 0, sum_nowp = 0;   // every component divided by its own size (:350) before they are added (:301-302)
    for (int c = 0; c < comps; ++c) {
      const int i = comps * r + c;
      sad_wp[c] = (int64_t)sums[2 * i] / n_samples[c];
      sad_nowp[c] = (int64_t)(sums[2 * i + 1] << d) / n_samples[c];
      sum_wp += sad_wp[c]; sum_nowp += sad_nowp[c];
    }
    // :305 -- 0 / 0 is NaN and NaN >= 0.99 is false: identical pictures keep their (identity) weights present; x / 0 is +inf and disables them
    const double ratio = (double)sum_wp / (double)sum_nowp;
    const int present = ratio >= 0.99 ? 0 : 1;   // DTHRESH (:46); :306-314: all components of the reference together
    for (int c = 0; c < comps; ++c) {
      const int i = comps * r + c, wgt = present ? weight[i] : 1 << d, off = present ? offset[i] : 0;
      wp[i] = {wgt, off * (1 << (bd - 8)), d, d ? 1 << (d - 1) : 0};
      if (!info) continue;
      hmme_wp_info& o = info[i];
      o.cur_dc_sum = stats[2 * c]; o.cur_ac = stats[2 * c + 1]; o.ref_dc_sum = stats[2 * (comps + i)]; o.ref_ac = stats[2 * (comps + i) + 1];
      o.sad_wp = sad_wp[c]; o.sad_nowp = sad_nowp[c];
      o.log2_denom = d; o.weight = wgt; o.offset = off;
      o.present = present;
      if (c == 0) {
        o.served_search = hmme_weight_check(bd, &wp[i], 0) == HMME_OK ? 1 : 0;
        o.served_refine = hmme_weight_check(bd, &wp[i], 1) == HMME_OK ? 1 : 0;
      } else {   // what predict_args / frame_checks ask of a component's weight in the hmme_predict_chroma_* calls
        char msg[256];
        o.served_search = o.served_refine = other_weight_eval(bd, &wp[i], nullptr, nullptr, msg, sizeof msg) == HMME_OK ? 1 : 0;
      }
    }
  }
}

// xEstimateWPParamSlice over planes the entry point has checked: planes[c] = component c of the current picture, planes[comps (1 + r) + c] =
// of reference r.  wp[comps r + c] and, where given, info[comps r + c]; nothing is written before the last wait has succeeded
int wp_estimate(hmme_ctx* ctx, const char* who, const hmme_plane* const* planes, int comps, int n_refs, int log2_denom_start, hmme_weight* wp,
                hmme_wp_info* info) {
  const int n_planes = comps * (1 + n_refs), n_pairs = comps * n_refs, bd = planes[0]->bit_depth;
  hipStream_t s = ctx->stream;
  int rc = collect_stats(ctx, planes, n_planes, s);   // xCalcACDCParamSlice of every plane that has not been through it since its last fill
  if (rc) return rc;
  int64_t stats[2 * hmme::kMaxSetPlanes], n_samples[3] = {};
  for (int c = 0; c < comps; ++c) n_samples[c] = (int64_t)planes[c]->width * planes[c]->height;
  for (int i = 0; i < n_planes; ++i) { stats[2 * i] = planes[i]->stats_dc; stats[2 * i + 1] = planes[i]->stats_ac; }
  int d, weight[hmme::kMaxSetPairs], offset[hmme::kMaxSetPairs];
  wp_parameters(stats, n_samples, comps, n_refs, bd, log2_denom_start, &d, weight, offset);

  // xCalcSADvalueWP with the estimated and with the default parameters of every (reference, component): one launch, one read of the planes for both
  hmme::MeWpSadSet a = {};
  for (int i = 0; i < n_pairs; ++i) {
    a.weight[i] = weight[i];
    a.offset[i] = offset[i] * (1 << (d + bd - 8));   // iOffset << iRealLog2Denom (:344)
    a.log2_denom[i] = d;
  }
  rc = planes_read_begin(ctx, planes, n_planes, s);
  if (rc) return rc;
  unsigned long long h[2 * hmme::kMaxSetPairs];
  unsigned long long* d_sums = ctx->buf[kWpEst].as<unsigned long long>() + kWpSetSad;
  hipError_t e = hipMemsetAsync(d_sums, 0, sizeof(unsigned long long) * 2 * n_pairs, s);
  if (e != hipSuccess) rc = fail(ctx, HMME_ERR_DEVICE, "%s: %s", who, hipGetErrorString(e));
  if (rc == HMME_OK) rc = launch_wp_sad_set(ctx, planes, planes + comps, comps, n_refs, a, d_sums, s);
  if (rc == HMME_OK && (e = hipMemcpyAsync(h, d_sums, sizeof(unsigned long long) * 2 * n_pairs, hipMemcpyDeviceToHost, s)) != hipSuccess)
    rc = fail(ctx, HMME_ERR_DEVICE, "%s: %s", who, hipGetErrorString(e));
  rc = planes_read_end(ctx, planes, n_planes, s, rc);
  if (rc) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(s));
  wp_select(stats, n_samples, comps, n_refs, bd, d, weight, offset, h, wp, info);
  return HMME_OK;
}

// what both entry points refuse of their planes: cur = the comps planes of the current picture, refs = comps per reference, all of this
// context, of one bit depth and of the current picture's size, Cb and Cr half of it each way (chroma_size: what the hmme_predict_chroma_*
// calls ask of their planes).  Fills planes[c] = cur[c], planes[comps (1 + r) + c] = refs[comps r + c]
int wp_estimate_args(hmme_ctx* ctx, const char* who, const hmme_plane* const* cur, const hmme_plane* const* refs, int comps, int n_refs,
                     const hmme_plane** planes) {
  if (!cur || !refs) return fail(ctx, HMME_ERR_ARG, "%s: null argument", who);
  if (n_refs < 1 || n_refs > hmme::kMaxRefs) return fail(ctx, HMME_ERR_ARG, "%s: %d references outside 1..%d", who, n_refs, hmme::kMaxRefs);
  const int n_planes = comps * (1 + n_refs);
  for (int i = 0; i < n_planes; ++i) {
    planes[i] = i < comps ? cur[i] : refs[i - comps];
    if (!planes[i]) return fail(ctx, HMME_ERR_ARG, "%s: null plane", who);
    if (planes[i]->ctx != ctx) return fail(ctx, HMME_ERR_ARG, "%s: plane belongs to another context", who);
  }
  const int w = planes[0]->width, h = planes[0]->height, bd = planes[0]->bit_depth;
  for (int i = 0; i < n_planes; i += comps) {
    if (planes[i]->width != w || planes[i]->height != h)
      return fail(ctx, HMME_ERR_ARG, "%s: reference %d is %d x %d, the current picture %d x %d", who, i / comps - 1, planes[i]->width, planes[i]->height, w, h);
    const int rc = comps == 3 ? chroma_size(ctx, who, planes + i + 1, 2, w, h) : HMME_OK;
    if (rc) return rc;
  }
  for (int i = 0; i < n_planes; ++i)
    if (planes[i]->bit_depth != bd) return fail(ctx, HMME_ERR_ARG, "%s: planes of %d and %d bits in one call", who, bd, planes[i]->bit_depth);
  return HMME_OK;
}
// what the two hooks below refuse of a call's shape
bool wp_hook_shape(const int64_t* n_samples, int comps, int n_refs, int bd, int d) {
  if (!n_samples || (comps != 1 && comps != 3) || n_refs < 1 || n_refs > hmme::kMaxRefs || bd < 8 || bd > 12 || d < 3 || d > 7) return false;
  for (int c = 0; c < comps; ++c)
    if (n_samples[c] < 1) return false;
  return true;
}
}  // namespace

int hmme_test_wp_parameters(const int64_t* stats, const int64_t* n_samples, int comps, int n_refs, int bit_depth, int log2_denom_start, int* log2_denom,
                            int* weight, int* offset) {
  if (!stats || !log2_denom || !weight || !offset || !wp_hook_shape(n_samples, comps, n_refs, bit_depth, log2_denom_start)) return HMME_ERR_ARG;
  wp_parameters(stats, n_samples, comps, n_refs, bit_depth, log2_denom_start, log2_denom, weight, offset);
  return HMME_OK;
}
int hmme_test_wp_select(const int64_t* stats, const int64_t* n_samples, int comps, int n_refs, int bit_depth, int log2_denom, const int* weight,
                        const int* offset, const uint64_t* sums, hmme_weight* out_wp, hmme_wp_info* out_info) {
  if (!stats || !weight || !offset || !sums || !out_wp || !wp_hook_shape(n_samples, comps, n_refs, bit_depth, log2_denom)) return HMME_ERR_ARG;
  wp_select(stats, n_samples, comps, n_refs, bit_depth, log2_denom, weight, offset, (const unsigned long long*)sums, out_wp, out_info);
  return HMME_OK;
}

int hmme_plane_stats(const hmme_plane* pl, int64_t* dc_sum, int64_t* ac) {
  if (!pl) return HMME_ERR_ARG;
  hmme_ctx* ctx = pl->ctx;
  if (!dc_sum || !ac) return fail(ctx, HMME_ERR_ARG, "hmme_plane_stats: null output");
  const int rc = collect_stats(ctx, &pl, 1, ctx->stream);
  if (rc) return rc;
  *dc_sum = pl->stats_dc; *ac = pl->stats_ac;
  return HMME_OK;
}

int hmme_wp_estimate(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* const* refs, int n_refs, int log2_denom_start, hmme_weight* out_wp,
                     hmme_wp_info* out_info) {
  static const char* const who = "hmme_wp_estimate";
  if (!ctx) return HMME_ERR_ARG;
  if (!out_wp) return fail(ctx, HMME_ERR_ARG, "%s: null output", who);
  if (log2_denom_start < 3 || log2_denom_start > 7) return fail(ctx, HMME_ERR_ARG, "%s: log2_denom_start %d outside 3..7", who, log2_denom_start);
  const hmme_plane* planes[hmme::kMaxRefs + 1];
  const int rc = wp_estimate_args(ctx, who, &cur, refs, 1, n_refs, planes);
  return rc ? rc : wp_estimate(ctx, who, planes, 1, n_refs, log2_denom_start, out_wp, out_info);
}

// the estimator joint over Y, Cb, Cr (the rule: include/hmme.h)
int hmme_wp_estimate_420(hmme_ctx* ctx, const hmme_plane* const* cur, const hmme_plane* const* refs, int n_refs, int log2_denom_start,
                         hmme_weight* out_wp_luma, hmme_weight* out_wp_chroma, hmme_wp_info* out_info) {
  static const char* const who = "hmme_wp_estimate_420";
  if (!ctx) return HMME_ERR_ARG;
  if (!out_wp_luma || !out_wp_chroma) return fail(ctx, HMME_ERR_ARG, "%s: null output", who);
  if (log2_denom_start < 3 || log2_denom_start > 7) return fail(ctx, HMME_ERR_ARG, "%s: log2_denom_start %d outside 3..7", who, log2_denom_start);
  const hmme_plane* planes[hmme::kMaxSetPlanes];
  int rc = wp_estimate_args(ctx, who, cur, refs, 3, n_refs, planes);
  if (rc) return rc;
  hmme_weight wp[hmme::kMaxSetPairs];
  rc = wp_estimate(ctx, who, planes, 3, n_refs, log2_denom_start, wp, out_info);
  if (rc) return rc;
  for (int r = 0; r < n_refs; ++r) {
    out_wp_luma[r] = wp[3 * r];
    out_wp_chroma[2 * r] = wp[3 * r + 1]; out_wp_chroma[2 * r + 1] = wp[3 * r + 2];
  }
  return HMME_OK;
}

namespace {
// hmme_test_time_*: `reps` runs of `first` and then, where given, `reps` runs of `second` on `s` between events -> the milliseconds of one
// run of each.  A run that fails ends the measurement with its code; what was enqueued has finished when this returns
int time_reps(hmme_ctx* ctx, hipStream_t s, int reps, const char* what, const std::function<int()>& first, float* first_ms,
              const std::function<int()>& second = nullptr, float* second_ms = nullptr) {
  const std::function<int()>* run[2] = {&first, &second};
  float* out[2] = {first_ms, second_ms};
  const int groups = second ? 2 : 1;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  float ms[2] = {0.f, 0.f};
  int rc = HMME_OK;
  hipError_t e = hipSuccess;
  for (int i = 0; i <= groups && e == hipSuccess; ++i) e = hipEventCreate(&ev[i]);
  if (e == hipSuccess) e = hipEventRecord(ev[0], s);
  for (int g = 0; g < groups && e == hipSuccess; ++g) {
    for (int i = 0; i < reps && rc == HMME_OK; ++i) rc = (*run[g])();
    e = hipEventRecord(ev[g + 1], s);
  }
  if (e == hipSuccess) e = hipEventSynchronize(ev[groups]);
  for (int g = 0; g < groups && e == hipSuccess; ++g) e = hipEventElapsedTime(&ms[g], ev[g], ev[g + 1]);
  for (hipEvent_t v : ev)
    if (v) hipEventDestroy(v);
  if (rc == HMME_OK && e != hipSuccess) rc = fail(ctx, HMME_ERR_DEVICE, "timing %s: %s", what, hipGetErrorString(e));
  for (int g = 0; g < groups && rc == HMME_OK; ++g) *out[g] = ms[g] / reps;
  return rc;
}
}  // namespace

int hmme_test_time_wp_estimate_passes(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* const* refs, int n_refs, const hmme_weight* wp, void* stream,
                                      int reps, float* stats_ms, float* sad_ms) {
  if (!ctx) return HMME_ERR_ARG;
  if (!wp || !stats_ms || !sad_ms || reps < 1 || wp->shift < 0 || wp->shift > 7) return fail(ctx, HMME_ERR_ARG, "hmme_test_time_wp_estimate_passes: bad argument");
  const hmme_plane* planes[hmme::kMaxRefs + 1];
  int rc = wp_estimate_args(ctx, "hmme_test_time_wp_estimate_passes", &cur, refs, 1, n_refs, planes);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  rc = planes_read_begin(ctx, planes, 1 + n_refs, s);
  if (rc) return rc;
  hmme::MeWpSadSet a = {};
  for (int r = 0; r < n_refs; ++r) { a.weight[r] = wp->w0; a.offset[r] = wp->offset * (1 << wp->shift); a.log2_denom[r] = wp->shift; }
  unsigned long long* d_sums = ctx->buf[kWpEst].as<unsigned long long>();
  const hipError_t e = hipMemsetAsync(d_sums, 0, sizeof(unsigned long long) * kWpSetWords, s);
  if (e != hipSuccess) rc = fail(ctx, HMME_ERR_DEVICE, "hmme_test_time_wp_estimate_passes: %s", hipGetErrorString(e));
  if (rc == HMME_OK)
    rc = time_reps(ctx, s, reps, "the estimator's passes", [&] { return launch_stats_set(ctx, planes, 1, d_sums, s); }, stats_ms,
                   [&] { return launch_wp_sad_set(ctx, planes, planes + 1, 1, n_refs, a, d_sums + kWpSetSad, s); }, sad_ms);
  return planes_read_end(ctx, planes, 1 + n_refs, s, rc);
}

int hmme_test_time_bipred_origin(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* other, const void* d_other_mv, int mv_per_ctu, void* stream,
                                 int reps, float* avg_ms) {
  if (!ctx) return HMME_ERR_ARG;
  if (!cur || !other || !d_other_mv || !avg_ms || reps < 1 || (mv_per_ctu != 1 && mv_per_ctu != 64)) return fail(ctx, HMME_ERR_ARG, "hmme_test_time_bipred_origin: bad argument");
  hmme_frame_params fp = {1, 0, cur->bit_depth, 0, -1};
  int rc = bi_check(ctx, "hmme_test_time_bipred_origin", &fp, 0);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  PairLaunch pl;
  rc = pairs_begin(ctx, &cur, &other, 1, &fp, s, &pl);
  if (rc) return rc;
  const WpGeom g(cur);
  rc = ensure(ctx, ctx->buf[kWp1], g.blk_bytes);
  const BiLaunch B = {&cur, nullptr, &other, 1, &other, 1, d_other_mv, nullptr, mv_per_ctu, nullptr, BiWp::unweighted(cur->bit_depth)};   // one pair, bias maxv
  const uint8_t* at;
  if (rc == HMME_OK)
    rc = time_reps(ctx, s, reps, "the origin pass", [&] { return bi_origin(ctx, B, 0, pl, BiOrigin::blocks(ctx, g, cur->ctus_x), s, &at); }, avg_ms);
  return pairs_end(ctx, &cur, &other, 1, s, rc);
}

int hmme_test_time_weight_passes(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* ref, const hmme_weight* wp, void* stream, int reps,
                                 float* ref_ms, float* cur_ms) {
  if (!ctx) return HMME_ERR_ARG;
  if (!cur || !ref || !wp || !ref_ms || !cur_ms || reps < 1) return fail(ctx, HMME_ERR_ARG, "hmme_test_time_weight_passes: bad argument");
  WpInfo info;
  char msg[256];
  int rc = weight_eval(ref->bit_depth, wp, 0, kPictureBlock, &info, msg, sizeof msg);
  if (rc) return fail(ctx, rc, "hmme_test_time_weight_passes: %s", msg);
  hmme_frame_params fp = {1, 0, ref->bit_depth, 0, -1};
  hipStream_t s = (hipStream_t)stream;
  PairLaunch pl;
  rc = pairs_begin(ctx, &cur, &ref, 1, &fp, s, &pl);
  if (rc) return rc;
  const WpGeom g(ref);
  rc = ensure(ctx, ctx->buf[kWp0], g.plane_bytes);
  if (rc == HMME_OK) rc = ensure(ctx, ctx->buf[kWp1], g.blk_bytes);
  if (rc == HMME_OK)
    rc = time_reps(ctx, s, reps, "the weighting passes", [&] { return weight_plane(ctx, ref, g, ctx->wp(0), wp->w0, wp->round, wp->shift, wp->offset + info.bias, s); },
                   ref_ms, [&] { return bias_blocks(ctx, cur, ctx->wp(1), info.bias, s); }, cur_ms);
  return pairs_end(ctx, &cur, &ref, 1, s, rc);
}

int hmme_test_time_search_kernel(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* ref, const hmme_frame_params* fp,
                            const void* d_pred_q, void* d_out_mv, void* d_out_sad, void* stream, int reps, float* avg_ms) {
  int first, count;
  int rc = check_frame_args(ctx, cur, ref, fp, &first, &count);
  if (rc) return rc;
  if (!avg_ms || reps < 1) return fail(ctx, HMME_ERR_ARG, "hmme_test_time_search_kernel: bad reps/avg_ms");
  hipStream_t s = (hipStream_t)stream;
  PairLaunch pl;
  rc = pairs_begin(ctx, &cur, &ref, 1, fp, s, &pl);
  if (rc || pl.count == 0) return rc;
  // job table once (it is not part of the timed kernel), then `reps` launches of the search kernel(s) alone
  const FramePlan plan = plan_launch(ctx, fp, count, 1);
  rc = prep_jobs(ctx, cur, fp, d_pred_q, first, count, 1, s, plan);
  if (rc == HMME_OK)
    rc = time_reps(ctx, s, reps, "the search kernel", [&] {
      return run_search(ctx, pl.cur_blocks, cur->ctus_x, pl.refs, ref->pitch, fp, plan, (int16_t*)d_out_mv, (uint32_t*)d_out_sad, s);
    }, avg_ms);
  return pairs_end(ctx, &cur, &ref, 1, s, rc);
}

}  // extern "C"
