// me_kernels.hpp -- hand-written HIP kernels (gfx950 / CDNA4) of the hmme engine.
//
// Hot kernel: me_search_kernel<FEN>.  One workgroup (256 threads = 4 waves) searches one CTU
// against one reference picture:
//   1. the (Wy+63) x (Wx+63) byte reference window is staged into LDS (coalesced dword loads,
//      re-aligned with v_alignbyte so that window column 0 sits at LDS byte 0 of each row);
//   2. waves pull *tasks* (a strip of candidate MVs) from an LDS counter.  In a task every lane
//      owns four horizontally adjacent candidates per iteration and walks the whole 64x64 CTU:
//      v_qsad_pk_u16_u8 leaves (current-block dwords arrive through scalar loads, i.e. as SGPR
//      operands), packed-u16 / linear-key reduction tree, per-lane min, wave butterfly --
//      generated straight-line code, see tools/gen_me_tree.py;
//   3. each wave folds its ten running-minimum registers into a per-CTU LDS table with 64-bit
//      (cost, y, x) keys (ds_min_u64) so that ties resolve in raster order like
//      TEncSearch::xPatternSearch's strict '<' (reference TEncSearch.cpp:3866-3889);
//   4. 593 (mv, sad) results are written out coalesced.
//
// No MFMA: this is integer absolute-difference work.  The kernel is VALU-bound.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hmme {

constexpr int kParts = 593;            // NUM_CTU_PARTS, reference TLibCommon/TypeDef.h:263
constexpr int kPDW = 49;               // LDS window pitch in dwords (196 B >= 129 + 63 + 3)
constexpr int kWinRowsMax = 192;       // (2*64+1) + 63
constexpr int kIdxBits = 10;           // key = cost << 10 | iter(2) | lane(6) | j(2)
constexpr uint32_t kInvCost = 3146751u;  // > any valid cost (<= 1047552 + 65535); + max SAD stays < 2^22
constexpr int kGroups = 10;
// lane-iterations per task (<= 4: 2 iteration bits in the key).  A task ends with the flush of ten running-minimum registers into the
// CTU's LDS table; whole-picture launches run 4 per task (measured on 2160p: 1 / 2 / 4 -> 3 252 / 3 256 / 3 284 GSAD/s,
// profiles/archive/r02f_*), split launches (one CTU dealt to many workgroups, where the number of tasks is the parallelism) 1: the per-CTU
// call at SR 64 goes from 9 to 17 workgroups of one iteration per wave, 0.086 -> 0.065 ms (profiles/archive/r02l_*)
constexpr int kIterPerTask = 4;
constexpr int kIterPerTaskSplit = 1;
static_assert(kIterPerTask == 4 && kIterPerTaskSplit <= 4, "2 iteration bits in the key; the guided schedule deals 4 / 2 / 1");
constexpr int kThreads = 256;

// one CTU search: everything in integer pels except the quarter-pel predictor
struct MeJob {
  int16_t ctu_x, ctu_y;   // CTU origin in the picture
  int16_t lt_x, lt_y;     // window top-left   (xSetSearchRange, reference TEncSearch.cpp:3814-3830)
  int16_t rb_x, rb_y;     // window bottom-right, inclusive
  int16_t pred_x, pred_y; // AMVP predictor, quarter pels
};
static_assert(sizeof(MeJob) == 16, "MeJob layout");
// CTU origins are multiples of 64, so the low 6 bits of MeJob::ctu_x carry the index of the picture pair the job belongs to: one
// launch searches up to 16 (current, reference) pairs -- several references of one picture (hmme_search_frame_multi: the same
// current plane in every entry) or several pictures of a sequence (hmme_search_pairs_device).  Both sets travel by value.
constexpr int kMaxRefs = 16;
struct RefSet { const uint8_t* base[kMaxRefs]; };

#include "me_slotmap.inc"
#include "me_slotmap3.inc"

// ---- helpers used by the generated tree ------------------------------------------------------
typedef uint16_t u16x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
// LDS reads of the generated tree are volatile: they are issued exactly where the generator put
// them (one 8x8 CU ahead of their use) instead of being hoisted and spilled by the scheduler
typedef __attribute__((address_space(3))) char lds_char_t;
typedef volatile __attribute__((address_space(3))) uint64_t lds_vu64_t;
typedef volatile __attribute__((address_space(3), aligned(4))) uint64_t lds_vu64a4_t;   // -> ds_read2_b32

// packed-u16 x4 sums never carry between halves (every partial SAD here is <= 65 280), so the packed add is
// a plain 64-bit add (one v_lshl_add_u64, ~4.6 cycles) and the packed subtract two 32-bit subtracts
// (v_sub_u32, ~2.7 cycles each) instead of two v_pk_*_u16 (~4.3 each)  [profiles/r01_valu_rates2_ubench.txt]
// The two subtracts are asm, and the pair they form is opaque: written in C++, a difference that goes on into `(p << 1) + pkm` was
// rewritten by the compiler, which cannot know that bit 31 of the low half is clear, into a borrow chain and masks (v_subb_co_u32,
// v_subrev_co_u32, v_and_b32 0x7fffffff: 272 instructions for 64 subtracts and their 64 adds where 192 are designed).
__device__ __forceinline__ uint64_t me_pkadd(uint64_t a, uint64_t b) { return a + b; }
__device__ __forceinline__ uint64_t me_pksub(uint64_t a, uint64_t b) {
  uint32_t lo, hi;
  asm volatile("v_sub_u32 %0, %1, %2" : "=v"(lo) : "v"((uint32_t)a), "v"((uint32_t)b));
  asm volatile("v_sub_u32 %0, %1, %2" : "=v"(hi) : "v"((uint32_t)(a >> 32)), "v"((uint32_t)(b >> 32)));
  uint64_t r = (uint64_t)hi << 32 | lo;
  asm volatile("" : "+v"(r));   // without it the shift of `(p << 1) + pkm` is split over the two halves again (32 v_lshlrev_b32 and as many moves)
  return r;
}

#define ME_MAXKEY 0xFFFFFFFFu
#define ME_QSAD(pair, cur, acc) __builtin_amdgcn_qsad_pk_u16_u8((pair), (cur), (acc))
// key_j = sad_j * mult + c_j : one v_mad_u32_u16 per candidate (op_sel picks the packed half)
#define ME_KEYS(v, p, mult)                                                                                    \
  uint32_t v##_0, v##_1, v##_2, v##_3;                                                                         \
  asm volatile("v_mad_u32_u16 %0, %1, %2, %3" : "=v"(v##_0) : "v"((uint32_t)(p)), "s"(mult), "v"(c0));                   \
  asm volatile("v_mad_u32_u16 %0, %1, %2, %3 op_sel:[1,0,0,0]" : "=v"(v##_1) : "v"((uint32_t)(p)), "s"(mult), "v"(c1));   \
  asm volatile("v_mad_u32_u16 %0, %1, %2, %3" : "=v"(v##_2) : "v"((uint32_t)((p) >> 32)), "s"(mult), "v"(c2));           \
  asm volatile("v_mad_u32_u16 %0, %1, %2, %3 op_sel:[1,0,0,0]" : "=v"(v##_3) : "v"((uint32_t)((p) >> 32)), "s"(mult), "v"(c3))
// keys are linear in the SAD:  K(a U b) = K(a) + K(b) - c ;  K(a \ b) = K(a) - K(b) + c
#define ME_LIN(v, a, b)                                                                                         \
  uint32_t v##_0, v##_1, v##_2, v##_3;                                                                          \
  asm volatile("v_add3_u32 %0, %1, %2, %3" : "=v"(v##_0) : "v"(a##_0), "v"(b##_0), "v"(nc0));                              \
  asm volatile("v_add3_u32 %0, %1, %2, %3" : "=v"(v##_1) : "v"(a##_1), "v"(b##_1), "v"(nc1));                              \
  asm volatile("v_add3_u32 %0, %1, %2, %3" : "=v"(v##_2) : "v"(a##_2), "v"(b##_2), "v"(nc2));                              \
  asm volatile("v_add3_u32 %0, %1, %2, %3" : "=v"(v##_3) : "v"(a##_3), "v"(b##_3), "v"(nc3))
// K(a) >= K(b) whenever b's rectangle is inside a's, so |K(a) - K(b)| + c is exact: one v_sad_u32
#define ME_SUB(v, a, b)                                                                                         \
  uint32_t v##_0, v##_1, v##_2, v##_3;                                                                          \
  asm volatile("v_sad_u32 %0, %1, %2, %3" : "=v"(v##_0) : "v"(a##_0), "v"(b##_0), "v"(c0));                                \
  asm volatile("v_sad_u32 %0, %1, %2, %3" : "=v"(v##_1) : "v"(a##_1), "v"(b##_1), "v"(c1));                                \
  asm volatile("v_sad_u32 %0, %1, %2, %3" : "=v"(v##_2) : "v"(a##_2), "v"(b##_2), "v"(c2));                                \
  asm volatile("v_sad_u32 %0, %1, %2, %3" : "=v"(v##_3) : "v"(a##_3), "v"(b##_3), "v"(c3))
// the key arithmetic above, this minimum and the masked merges below are `asm volatile`: not for side effects but to keep
// their mutual order in the ISA equal to the generator's order, which places every masked merge >= 2 of these instructions
// after the ones that produce its inputs (tools/gen_me_tree.py space_merges)
__device__ __forceinline__ uint32_t me_min4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  uint32_t r;
  asm volatile("v_min3_u32 %0, %1, %2, %3\n\tv_min_u32 %0, %0, %4" : "=&v"(r) : "v"(a), "v"(b), "v"(c), "v"(d));
  return r;
}
#define ME_MIN4(k) me_min4(k##_0, k##_1, k##_2, k##_3)
// A difference K(a \\ b) is read by nothing but the minimum of its own slot (the right 4x8 half of an 8x8 CU, 12x16, 24x32, 48x64, ...;
// a and b keys of ONE family, b inside a): the four keys and their minimum as one asm block of six instructions.  hipcc pads an asm block
// that reads what the asm block right before it wrote (s_nop), never inside one; the four keys live in two scratch registers.
#define ME_SUBMIN4(r, a, b)                                                                                     \
  uint32_t r;                                                                                                   \
  {                                                                                                             \
    uint32_t r##_t, r##_u;                                                                                      \
    asm volatile("v_sad_u32 %0, %3, %7, %11\n\tv_sad_u32 %1, %4, %8, %12\n\tv_sad_u32 %2, %5, %9, %13\n\t"            \
                 "v_min3_u32 %0, %0, %1, %2\n\tv_sad_u32 %1, %6, %10, %14\n\tv_min_u32 %0, %0, %1"                    \
                 : "=&v"(r), "=&v"(r##_t), "=&v"(r##_u)                                                        \
                 : "v"(a##_0), "v"(a##_1), "v"(a##_2), "v"(a##_3), "v"(b##_0), "v"(b##_1), "v"(b##_2), "v"(b##_3), "v"(c0), "v"(c1),     \
                   "v"(c2), "v"(c3));                                                                           \
  }

// Packed minimum (the PK twin of the search kernel, me_tree_pk_fen*.inc): a slot of an 8x8 CU -- 8x4, 4x8, 8x8: all-row sums of at most
// kPkSlotMax -- whose packed sums p feed nothing as keys takes the minimum over the lane's four candidates on packed u16 COSTS:
//   q = p + pkm        one 64-bit add (the compiler's v_lshl_add_u64); pkm = the four MV costs, kPkMarker where a candidate is invalid
//   m = min of q's four fields    two v_pk_min_u16 (the second one reads the first one's two halves through op_sel)
//   key = m * 1024 + ctag         one v_mad_u32_u16; ctag = iteration | lane << 2, j = 0
// 4 instructions where ME_KEYS + ME_MIN4 are 6.  The key says which QUAD won, not which of its four candidates: me_pk_recover finds that
// once per slot and job.  Exact while every valid cost + sum stays below the marker and the marker + any sum below 2^16: me_pk_gate decides
// per launch (hmme.hip launch_search8).  An invalid candidate loses by value; a lane whose four candidates are all invalid carries
// kInvCost << 10 in ctag, so ME_FLUSH drops it like any other invalid key.  The three instructions are one asm block (nothing padded
// inside it; the first reads what the compiler's add wrote, which the compiler pads if it must).
constexpr uint32_t kPkSlotMax = 64 * 255;                 // 16 320: the 8x8 CU, every sample difference 255
constexpr uint32_t kPkMarker = 0xFFFFu - kPkSlotMax;      // 49 215: marker + any sum fits u16
// The MV cost of a launch is at most (lambda_q16 * bits) >> 16 with bits <= 2 * 37: window and predictor components are int16 (integer
// and quarter pels), so a component's difference is below 2^18 in quarter pels and me_component_bits at most 2 * 18 + 1.  The packed
// path runs only where that bound + kPkSlotMax stays below the marker (and the product does not wrap uint32, or `cost` would be no bound).
constexpr uint32_t kPkMaxBits = 2 * 37;
__host__ __device__ inline bool me_pk_gate(uint32_t lambda_q16) {
  const uint64_t prod = (uint64_t)lambda_q16 * kPkMaxBits;
  return prod <= 0xFFFFFFFFull && (prod >> 16) + kPkSlotMax < kPkMarker;
}
// Marker-free packed minima (PK = 2; FEN 1 only; the bounds of the full-task twin below, which is the body that runs them -- the marker-free
// tree itself, tools/gen_me_tree.py Tree(1, pk=2), is that body's yardstick and no longer part of the kernel): the marker exists for the invalid candidates of a PARTLY valid lane, and
// such lanes exist only where a window row's last quad is cut (wx % 4 != 0): in the part that holds that quad, and in the folded
// iteration of the 32-quad part (me_task_marker_free).  Every other task has only lanes that are wholly valid -- pkm holds four real MV
// costs -- or wholly invalid -- kInvCost << 10 in ctag drops the lane whatever its packed fields hold, carries between them included.
// Without a marker a packed cost only has to stay below 2^16, and twelve of the thirteen slots of a 16x16 CU do: 16x4, 4x16 <= 16 320,
// 16x8, 8x16 <= 32 640, 16x12, 12x16 <= kPk2SlotMax, + an MV cost of at most 0xFFFF - kPk2SlotMax (me_pk2_gate).  They take ME_PKMIN
// there, ME_PKMINE where FEN halves the rows (h > 8): the 64-bit add that adds the packed MV costs doubles the even-row sums on the way
// (v_lshl_add_u64; an even-row sum is at most 24 480, the shift stays inside its u16 field).  min * 1024 + ctag stays inside the key:
// 65 535 * 1024 + (kInvCost << 10 | 1023) < 2^32.  Tasks with a partly valid lane run the PK = 1 body in the same kernel, and so do
// marker-free tasks with a lane outside the window (a part's last, partial lane-iteration on a clipped window): me_task_full.
constexpr uint32_t kPk2SlotMax = 16 * 12 * 255;           // 48 960: 16x12 / 12x16, every sample difference 255
__host__ __device__ inline bool me_pk2_gate(uint32_t lambda_q16) {
  const uint64_t prod = (uint64_t)lambda_q16 * kPkMaxBits;
  return prod <= 0xFFFFFFFFull && (prod >> 16) + kPk2SlotMax <= 0xFFFFu;
}
// which body an 8-bit search launch runs: 0 the 32-bit tree, 1 the packed-minimum twin, 2 the kernel that holds the twin and the full-task
// body.  FEN 0 stays on 1: its tall-family sums are all-row sums of twice the rows, its recovery would read 16 rows per slot, and no
// benchmark or encoder configuration runs it
__host__ __device__ inline int me_pk_body(uint32_t lambda_q16, int fen) {
  return (fen && me_pk2_gate(lambda_q16)) ? 2 : me_pk_gate(lambda_q16) ? 1 : 0;
}
// whether the task (part k, lane-iterations it0 .. it0 + n_it - 1) of a wx x wy window has no partly valid lane.  The last quad of a
// row lies in the part of the lowest set bit of `quads`; with the fold, the leftover quads of the last window row are also met in the
// second lane row of the 32-quad part's last iteration (rows wy - 1 and wy: wy is odd)
__host__ __device__ inline bool me_task_marker_free(int wx, int wy, int k, int it0, int n_it) {
  if (!(wx & 3)) return true;
  const int quads = (wx + 3) >> 2;
  if ((quads & -quads) == (1 << k)) return false;
  const bool fold = (quads & 32) && (quads & 31) && (wy & 1);   // me_fold (below)
  return !(fold && k == 5 && 2 * (it0 + n_it) > wy);
}
// whether the task runs the full-task twin: a part of at least four quads (k >= 2) that does not hold the row's cut quad, and every lane
// of every one of its lane-iterations inside the part's rows (the folded iteration of the 32-quad part is not: its second lane row lies
// below the window).  Every lane is then valid with all four candidates
__host__ __device__ inline bool me_task_full(int wx, int wy, int k, int it0, int n_it) {
  if (k < 2) return false;
  const int quads = (wx + 3) >> 2;
  if ((wx & 3) && (quads & -quads) == (1 << k)) return false;
  const bool fold = (quads & 32) && (quads & 31) && (wy & 1);   // me_fold (below)
  return (it0 + n_it) * (64 >> k) <= ((k == 5 || !fold) ? wy : wy - 1);
}
// Packed running minima carried across the full tasks of one part (whole-job launches): the ten low bits of their keys hold the ABSOLUTE
// lane-iteration above the 16-candidate group inside it, it_abs(6) | lane_now[5:2](4), where the per-task keys hold it - it0 (2 bits), the
// same four group bits and two zeros.  A group of part k lies at (row, group in the row): a lane-iteration covers 64 >> k rows of
// 2^(k-2) groups, so the index is (row / ty) << 4 | (row % ty) << (k - 2) | group -- its integer order is the raster order of the part,
// and a wave's minima over any number of full tasks of one part decode without the task's it0.  Six bits hold every iteration of a full
// task: its rows end inside a window of at most 129 rows and a lane-iteration has at least two (me_task_carry_fits).
constexpr int kCarryGroupBits = 4, kCarryItBits = kIdxBits - kCarryGroupBits;
__host__ __device__ inline bool me_task_carry_fits(int wx, int wy, int k, int it0, int n_it) {
  return !me_task_full(wx, wy, k, it0, n_it) || it0 + n_it <= (1 << kCarryItBits);
}
__host__ __device__ inline uint32_t me_carry_index(int k, int row, int group) {
  const int ty = 64 >> k;
  return (uint32_t)((row / ty) << kCarryGroupBits | (row % ty) << (k - 2) | group);
}
__host__ __device__ inline void me_carry_position(int k, uint32_t index, int& row, int& group) {
  const int g4 = (int)(index & ((1u << kCarryGroupBits) - 1));
  row = (int)(index >> kCarryGroupBits) * (64 >> k) + (g4 >> (k - 2));
  group = g4 & ((1 << (k - 2)) - 1);
}
#define ME_PKMIN(r, p) ME_PKMIN_Q(r, (p) + pkm)
#define ME_PKMINE(r, p) ME_PKMIN_Q(r, ((p) << 1) + pkm)
#define ME_PKMIN_Q(r, q)                                                                                        \
  uint32_t r;                                                                                                   \
  {                                                                                                             \
    const uint64_t r##_q = (q);                                                                                 \
    asm volatile("v_pk_min_u16 %0, %1, %2\n\tv_pk_min_u16 %0, %0, %0 op_sel:[0,1] op_sel_hi:[1,0]\n\t"                \
                 "v_mad_u32_u16 %0, %0, %3, %4"                                                                 \
                 : "=&v"(r) : "v"((uint32_t)r##_q), "v"((uint32_t)(r##_q >> 32)), "s"(mult_a), "v"(ctag));      \
  }

// Full-task twin (PK = 2, me_tree_pk4_fen1.inc): the body of the tasks whose lanes ALL lie inside the window (me_task_full) -- for the
// 129 x 129 window the 64 lane-iterations of the 32-quad part that come before the folded one.  Their lane layout puts the two lowest
// bits of the quad index into lane bits 5 and 4: lanes l, l ^ 16, l ^ 32, l ^ 48 hold four adjacent quads, 16 contiguous candidates of
// one window row starting at a multiple of 16 (every part with k >= 2 starts on one).  The two butterfly levels on those lane bits then
// merge candidates that one key can stand for, so they run BEFORE the key exists, on the u16 minima themselves:
//   ME_PKMIN16_LO / _HI   q = p + pkm (one 64-bit add), v_pk_min_u16 of its halves, and one v_min_u16_sdwa that writes the minimum of that
//                         result's two halves into the low / high half of a register shared with the next packed slot
//   me_pmerge2 / 3        v_permlane32_swap / v_permlane16_swap of two such registers + v_pk_min_u16: two slots per register merged in the
//                         two instructions that merge one on keys
//   ME_KEY16_LO / _HI     key = half * 1024 + ctag, one v_mad_u32_u16 per half, a quarter as many as ME_PKMIN forms.  ctag names the
//                         16-candidate group (its first quad): me_pk_recover finds the candidate.
// MV costs carried in the sums (tools/gen_me_tree.py Tree(1, pk=4); Tree(1, pk=3), the same body without the carry, stays there as the
// yardstick): every lane of a full task is valid, so pkm holds four real costs, and a packed sum that contains pkm exactly once IS the
// slot's packed cost.  The left 8x8 CUs of a 16x16 region add pkm to one leaf sum (top CU: its top-left block, bottom CU: its bottom-left
// block); their 8x4 / 4x8 / 8x8 sums that contain that block and the region's 16x8 and 16x4 sums go into ME_PKMIN16_* as they stand --
// 10 of the region's 24 all-rows slots pay no add of their own, for two adds of pkm.  No value exceeds what P + pkm reached: the gate and
// every bound above stay.  The 16x8 strip a region hands to its 32x32 (two of them reach 65 280 and become keys) gives the costs back
// with one add of npkm, the 64-bit negation of pkm: no field borrows, each holds at least its cost.
// The four levels on lane bits 3..0 follow on keys as in every body.  Ties between groups are settled by (cost, iteration, ly, lx >> 2),
// the raster order, as they are between quads in the other bodies: the key's lane field is ly << k | lx, not the physical lane.
// Every lane of a full task is valid: no marker, no invalid cost in ctag, and the marker-free body's bounds hold (me_pk2_gate).
// v_permlane*_swap wants 2 wait states after a VALU write of either operand, like a DPP read: the generator spaces the merges from their
// producers (space_merges) and pads the rest (s_nop 1); the SDWA write of a register half is followed by at least one other instruction
// before anything reads the register (the _HI form computes its v_pk_min_u16 in between).
#define ME_PKMIN16_LO(r, q)                                                                                     \
  uint32_t r;                                                                                                   \
  {                                                                                                             \
    const uint64_t r##_q = (q);                                                                                 \
    asm volatile("v_pk_min_u16 %0, %1, %2\n\t"                                                                  \
                 "v_min_u16_sdwa %0, %0, %0 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:WORD_1" \
                 : "=&v"(r) : "v"((uint32_t)r##_q), "v"((uint32_t)(r##_q >> 32)));                              \
  }
#define ME_PKMIN16_HI(r, q)                                                                                     \
  {                                                                                                             \
    const uint64_t r##_q = (q);                                                                                 \
    uint32_t r##_t;                                                                                             \
    asm volatile("v_pk_min_u16 %1, %2, %3\n\t"                                                                  \
                 "v_min_u16_sdwa %0, %1, %1 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_0 src1_sel:WORD_1" \
                 : "+v"(r), "=&v"(r##_t) : "v"((uint32_t)r##_q), "v"((uint32_t)(r##_q >> 32)));                 \
  }
#define ME_KEY16_LO(k, r) uint32_t k; asm volatile("v_mad_u32_u16 %0, %1, %2, %3" : "=v"(k) : "v"(r), "s"(mult_a), "v"(ctag))
#define ME_KEY16_HI(k, r) uint32_t k; asm volatile("v_mad_u32_u16 %0, %1, %2, %3 op_sel:[1,0,0,0]" : "=v"(k) : "v"(r), "s"(mult_a), "v"(ctag))
#define ME_PMERGE(NAME, PAD, SWAP)                                                                           \
  __device__ __forceinline__ uint32_t NAME(uint32_t a, uint32_t b) {                                         \
    asm volatile(PAD SWAP " %0, %1\n\tv_pk_min_u16 %0, %0, %1" : "+v"(a), "+v"(b));                          \
    return a;                                                                                                \
  }
ME_PMERGE(me_pmerge2, "s_nop 1\n\t", "v_permlane32_swap_b32")      // role = lane bit 5
ME_PMERGE(me_pmerge3, "s_nop 1\n\t", "v_permlane16_swap_b32")      // role = lane bit 4
ME_PMERGE(me_pmerge2_nn, "", "v_permlane32_swap_b32")
ME_PMERGE(me_pmerge3_nn, "", "v_permlane16_swap_b32")

// butterfly transpose-reduce: merge two slot registers into one; lanes whose role bit is 0 keep
// slot a (min over the lane pair), lanes whose role bit is 1 keep slot b.
// Levels 0/1 (447 of the 588 merges): two DPP mins, the second one bank-masked so that it only
// overwrites the role-0 lanes.  s_nop 1 = the 2 wait states a DPP read needs after a VALU write of its
// source (hipcc does not pad hazards inside an asm statement).
// The _nn variants carry no padding: tools/gen_me_tree.py (space_merges) emits them only where >= 3 other ops separate the
// merge from the ops that produce its inputs, and tools/check_dpp_hazard.py verifies the distance in the final ISA (make check-isa).
#define ME_MERGE_DPP_MASKED(NAME, PAD, CTRL, MASK0)                                                          \
  __device__ __forceinline__ uint32_t NAME(uint32_t a, uint32_t b) {                                         \
    uint32_t r;                                                                                              \
    asm volatile(PAD "v_min_u32_dpp %0, %2, %2 " CTRL " row_mask:0xf bank_mask:0xf\n\t"                     \
        "v_min_u32_dpp %0, %1, %1 " CTRL " row_mask:0xf bank_mask:" MASK0                                    \
        : "=&v"(r) : "v"(a), "v"(b));                                                                        \
    return r;                                                                                                \
  }
ME_MERGE_DPP_MASKED(me_merge0, "s_nop 1\n\t", "row_ror:8", "0x3")          // role = lane bit 3: lanes 0-7 of a row = banks 0,1
ME_MERGE_DPP_MASKED(me_merge1, "s_nop 1\n\t", "row_half_mirror", "0x5")    // role = lane bit 2: lanes 0-3, 8-11 = banks 0,2
ME_MERGE_DPP_MASKED(me_merge0_nn, "", "row_ror:8", "0x3")
ME_MERGE_DPP_MASKED(me_merge1_nn, "", "row_half_mirror", "0x5")
__device__ __forceinline__ uint32_t me_merge2(uint32_t a, uint32_t b) {   // role = lane bit 5
  u32x2_t r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
  return min(r.x, r.y);
}
__device__ __forceinline__ uint32_t me_merge3(uint32_t a, uint32_t b) {   // role = lane bit 4
  u32x2_t r = __builtin_amdgcn_permlane16_swap(a, b, false, false);
  return min(r.x, r.y);
}
template <int DPP_CTRL>
__device__ __forceinline__ uint32_t me_merge_dpp(uint32_t a, uint32_t b, bool role) {
  const uint32_t keep = role ? b : a;
  const uint32_t give = role ? a : b;
  return min(keep, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)give, DPP_CTRL, 0xf, 0xf, false));
}
#define me_merge4(a, b, role) me_merge_dpp<0x4E>(a, b, role)    // quad_perm [2,3,0,1] role = lane bit 1
#define me_merge5(a, b, role) me_merge_dpp<0xB1>(a, b, role)    // quad_perm [1,0,3,2] role = lane bit 0

// TComRdCost::xGetComponentBits (reference TComRdCost.cpp:278-292) in closed form
__device__ __forceinline__ uint32_t me_component_bits(int v) {
  const uint32_t t = (v <= 0) ? ((uint32_t)(-v) << 1) + 1u : ((uint32_t)v << 1);
  return 2u * (31u - (uint32_t)__builtin_clz(t)) + 1u;
}
// The same, and a negation, without a subtract instruction (v_xad_u32: (a ^ b) + c): for the prologue of a full task's lane-iteration,
// which shares the full-task body's basic block -- the block's v_sub_u32 are the two per packed subtract of the tree and no other
// (tests/test_search_isa.py counts them).  ~(2v) + 2 = 1 - 2v
__device__ __forceinline__ uint32_t me_neg_xad(uint32_t x) {
  uint32_t r;
  asm("v_xad_u32 %0, %1, -1, 1" : "=v"(r) : "v"(x));
  return r;
}
__device__ __forceinline__ uint32_t me_component_bits_xad(int v) {
  const uint32_t v2 = (uint32_t)v << 1;
  uint32_t t;
  asm("v_xad_u32 %0, %1, -1, 2" : "=v"(t) : "v"(v2));
  return 2u * (31u - (uint32_t)__builtin_clz(v > 0 ? v2 : t)) + 1u;
}
// TComRdCost::getCost(x, y) with cost scale 2 (reference TComRdCost.h:172-189): uint32 wrap, >> 16
__device__ __forceinline__ uint32_t me_mv_cost(uint32_t lambda_q16, int x, int y, int pred_x, int pred_y) {
  return (lambda_q16 * (me_component_bits((x << 2) - pred_x) + me_component_bits((y << 2) - pred_y))) >> 16;
}

// The slots that take the packed minimum in the PK twin (ME_PKMIN) and their rectangles in the CTU: 8x4 halves 0..127, 4x8 halves
// 128..255, 8x8 CUs 384..447 (tools/gen_me_tree.py slot_2NxN / slot_Nx2N / slot_2Nx2N at size 8).  WIDE (PK = 2): also the twelve slots
// of every 16x16 CU that the full-task body packs -- the AMP slots 256..383 (16x4, 16x12, 4x16, 12x16), 16x8 448..479, 8x16 480..511
__device__ __forceinline__ bool me_pk_slot(int s, bool wide, int& x, int& y, int& w, int& h) {
  if (s < 128) { x = (s & 7) * 8; y = (s >> 4) * 8 + ((s >> 3) & 1) * 4; w = 8; h = 4; return true; }
  if (s < 256) { x = ((s >> 1) & 7) * 8 + (s & 1) * 4; y = ((s - 128) >> 4) * 8; w = 4; h = 8; return true; }
  if (s >= 384 && s < 448) { x = (s & 7) * 8; y = ((s - 384) >> 3) * 8; w = 8; h = 8; return true; }
  if (!wide) return false;
  if (s < 384) {
    const int kk = (s - 256) >> 4;                       // 0, 1: 16x4 top / bottom; 2, 3: 16x12; 4, 5: 4x16 left / right; 6, 7: 12x16
    x = (s & 3) * 16; y = ((s >> 2) & 3) * 16; w = 16; h = 16;
    if (kk < 4) { h = kk < 2 ? 4 : 12; if (kk & 1) y += 16 - h; }
    else { w = kk < 6 ? 4 : 12; if (kk & 1) x += 16 - w; }
    return true;
  }
  if (s < 480) { x = (s & 3) * 16; y = ((s - 448) >> 3) * 16 + ((s >> 2) & 1) * 8; w = 16; h = 8; return true; }
  if (s < 512) { x = ((s >> 1) & 3) * 16 + (s & 1) * 8; y = ((s - 480) >> 3) * 16; w = 8; h = 16; return true; }
  return false;
}
// PK twin: a packed slot's entry v = (cost, y, x of the winning quad's first candidate) of the workgroup's table -> the same entry with
// the x of the winning candidate.  The slot's SAD is computed again for the quad's (up to four) valid candidates from the window still
// in LDS and the job's current block; the FIRST j whose SAD + MV cost equals the minimum wins, as xPatternSearch's strict '<' has it
// inside a row.  Between quads the order was settled by (cost, y, x of the quad), which is the raster order: quads do not overlap.
// About 0.1 % of a job's absolute differences.  A quad starts on a window dword and a slot on a current-block dword (both x are multiples
// of 4), so a row is RW / 4 + 1 window dwords and RW / 4 current-block dwords; four current-block bytes against the four candidates at once
// through the leaves' own v_qsad_pk_u16_u8 on window dword pairs (k, k + 1), each pair read on its own as the body reads them (one
// instruction per dword where v_alignbyte_b32 + v_sad_u8 per candidate were seven; a slot's sum is at most 32 640 here: packed u16);
// every load of the slot is issued before the first is used (one round trip: a workgroup of a segment launch runs a few
// lane-iterations per job, and a byte-wise loop with a load per row cost it 3 %).
// NR rows, STEP apart: STEP = 2 reads the even rows of a slot taller than 8 under FEN (its cost is twice their sum).
// PK = 2 (WIDE): a full task's entry names a 16-candidate GROUP -- x is its first quad's, a multiple of 16 -- so an entry with
// (x & 12) == 0 is recomputed for the group's up to four quads (those that start below wx; dwords (x + rx) / 4 .. + 3 + rw / 4 <= 48 of
// the row's 49), the first candidate whose cost is the minimum wins.  Such an entry may also come from the PK = 1 body (a quad that
// happens to be the first of its group; with the winner's j where the slot has 32-bit keys there).  Scanning the whole group is right for
// it too: an equal-cost valid candidate EARLIER in the same row would have been flushed by its own task with a smaller x and would have
// won the atomicMin (in a SPLIT launch: the later merge into g_best), so there is none before the entry's own quad; inside that quad the
// key minimum took the smallest j of the lane's equal costs, which is the first j found here; and the scan stops at the first match,
// which is therefore the entry's own candidate.  Every other entry keeps its quad's four candidates.
template <int RW, int NR, int STEP>
__device__ __forceinline__ void me_pk_sads(const uint32_t* wrow, int pdw, const uint8_t* __restrict__ crow, uint32_t sad[4]) {
  constexpr int ND = RW / 4;
  static_assert(RW * NR * 255 <= 0xFFFF, "the four sums are packed u16");
  typedef uint64_t __attribute__((aligned(4))) u64a4_t;
  uint32_t c[NR][ND];
  uint64_t d[NR][ND];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
#pragma unroll
    for (int k = 0; k < ND; ++k) c[r][k] = *(const uint32_t*)(crow + r * STEP * 64 + 4 * k);
#pragma unroll
    for (int k = 0; k < ND; ++k) d[r][k] = *(const u64a4_t*)(wrow + r * STEP * pdw + k);   // dwords k, k + 1: a register pair of its own
  }
  uint64_t acc = 0;
#pragma unroll
  for (int r = 0; r < NR; ++r)
#pragma unroll
    for (int k = 0; k < ND; ++k) acc = ME_QSAD(d[r][k], c[r][k], acc);
#pragma unroll
  for (int j = 0; j < 4; ++j) sad[j] = (uint32_t)(acc >> (16 * j)) & 0xFFFFu;
}
template <bool WIDE>
__device__ __forceinline__ unsigned long long me_pk_recover(unsigned long long v, int s, const uint32_t* win, int pdw, const uint8_t* __restrict__ cur_blk,
                                                            const MeJob& job, int wx, uint32_t lambda_q16) {
  int rx, ry, rw, rh;
  if (v == ~0ull || !me_pk_slot(s, WIDE, rx, ry, rw, rh)) return v;
  const int x_first = (int)(v & 0xfffc), y = (int)((v >> 16) & 0xffff);
  const uint32_t cost = (uint32_t)(v >> 32);
  const uint8_t* crow = cur_blk + ry * 64 + rx;
  const uint32_t by = me_component_bits(((job.lt_y + y) << 2) - job.pred_y);
  const int x_end = (WIDE && !(x_first & 12)) ? min(x_first + 16, wx) : x_first + 4;   // a group of a full task, or one quad
  v &= ~0xffffull;
#pragma unroll 1
  for (int xq = x_first; xq < x_end; xq += 4) {
  const uint32_t* wrow = win + (y + ry) * pdw + ((xq + rx) >> 2);   // dwords (xq + rx) / 4 .. + rw / 4 <= 48 of a 49-dword row
  uint32_t sad[4] = {0u, 0u, 0u, 0u};
  int sh = 0;
  if (!WIDE || max(rw, rh) <= 8) {
    if (rh == 4) me_pk_sads<8, 4, 1>(wrow, pdw, crow, sad);
    else if (rw == 4) me_pk_sads<4, 8, 1>(wrow, pdw, crow, sad);
    else me_pk_sads<8, 8, 1>(wrow, pdw, crow, sad);
  } else if (rh <= 8) {                                   // 16x4, 16x8: all rows
    if (rh == 4) me_pk_sads<16, 4, 1>(wrow, pdw, crow, sad);
    else me_pk_sads<16, 8, 1>(wrow, pdw, crow, sad);
  } else {                                                // taller than 8 (WIDE is FEN 1): even rows, twice their sum
    sh = 1;
    if (rh == 12) me_pk_sads<16, 6, 2>(wrow, pdw, crow, sad);
    else if (rw == 4) me_pk_sads<4, 8, 2>(wrow, pdw, crow, sad);
    else if (rw == 8) me_pk_sads<8, 8, 2>(wrow, pdw, crow, sad);
    else me_pk_sads<12, 8, 2>(wrow, pdw, crow, sad);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (xq + j < wx && (sad[j] << sh) + ((lambda_q16 * (me_component_bits(((job.lt_x + xq + j) << 2) - job.pred_x) + by)) >> 16) == cost) return v | (unsigned long long)(xq + j);
  }
  return v | (unsigned long long)x_first;
}

// 16-bit kernel (three candidates per lane, one lane-iteration per task): key = cost << 8 | lane(6) | j(2).  The 24-bit cost field
// holds HM's shifted sums with bi-prediction origins (<= 3 142 656 + 65 535) and the unshifted ones of
// hmme_search_params::shift_free (what cl/sad.cl computes: 10-bit <= 4 190 208 + 65 535, 9-bit bi-prediction origins
// <= 6 279 168 + 65 535; wider content when the samples of the call bound the sum below the marker, hmme.hip ctu_call); the invalid
// marker + the largest sum an invalid lane can add (< 8 000 000) stays < 2^24
constexpr int kIdxBits16 = 8;
constexpr uint32_t kInvCost16 = 8000000u;
constexpr int kThreads16 = 256;

// a CTU search cut into several workgroups: the 16-bit path cuts by candidate rows (LDS capacity), the 8-bit path
// by task range (latency of the per-CTU drop-in call, small pictures)
struct MeJob16 {
  MeJob j;
  int16_t y0, y1;      // 16-bit path: candidate rows [y0, y1); 8-bit split mode: tasks [y0, y1)
  int32_t job;         // index into the result arrays
};

// XCD-aware order of a launch's workgroups.  The dispatcher deals workgroup p of a grid to XCD p % 8, and each of the 8 XCDs has its own
// 4 MB L2.  The windows of neighbouring CTUs overlap by two thirds (192 of 192 + 64 columns, likewise rows): if neighbours run on the
// same XCD at about the same time their windows come out of that L2 instead of HBM.  So the N units of work of a launch (CTU searches
// in raster order, or their strips) are cut into 8 contiguous bands, and the p-th workgroup takes unit number (p >> 3) of band (p & 7):
// unit q <-> position p are a bijection on [0, N).  Results do not depend on it (every unit carries / derives its own output index).
__host__ __device__ inline int me_xcd_unit(int p, int n) {          // position -> unit
  const int x = p & 7, base = n >> 3, rem = n & 7;
  return x * base + (x < rem ? x : rem) + (p >> 3);
}
__host__ __device__ inline int me_xcd_position(int q, int n) {      // unit -> position
  const int base = n >> 3, rem = n & 7, big = rem * (base + 1);
  if (q < big) return (q % (base + 1)) * 8 + q / (base + 1);
  const int r = q - big;                                             // base >= 1 here: q >= big means some band has `base` units
  return (r % base) * 8 + rem + r / base;
}

// number of tasks me_search_kernel makes out of a wx x wy window (same arithmetic on host and device; the default is the split
// kernel's task size: host code and the prep kernels only count tasks for split launches)
// "fold": with 33 quads per row (the 129-wide window) and an odd number of rows, the 32-quad part's last iteration has an
// idle second row of lanes; its first lanes take the leftover quads of the LAST window row, so the narrow parts stop one
// row earlier (129 rows: 2 iterations of 64 rows instead of 3)
__host__ __device__ inline bool me_fold(int quads, int wy) { return (quads & 32) && (quads & 31) && (wy & 1); }
__host__ __device__ inline int me_num_tasks(int wx, int wy, int iter_per_task = kIterPerTaskSplit) {
  const int quads = (wx + 3) >> 2;
  const int wy_low = me_fold(quads, wy) ? wy - 1 : wy;
  int n = 0;
  for (int k = 5; k >= 0; --k)
    if (quads & (1 << k)) n += (((k == 5 ? wy : wy_low) + (64 >> k) - 1) / (64 >> k) + iter_per_task - 1) / iter_per_task;
  return n;
}
static_assert(sizeof(MeJob16) == 24, "MeJob16 layout");

// Task sizes of a whole-picture launch ("guided"): the lane-iterations of a part are dealt out 4 at a time while more than T4 (8)
// remain, then 2 at a time while more than T2 (2) remain, the last ones singly.  Large tasks keep the number of flushes low, small last ones keep the four waves of a
// workgroup level when the task counter runs dry (a wave that finishes a 4-iteration task early leaves its SIMD slot empty until the
// whole workgroup is done).  n4 / n2 / n1 = number of tasks of each size for `iters` iterations.
constexpr int kGuidedT4 = 8, kGuidedT2 = 2;
__host__ __device__ inline void me_guided(int iters, int& n4, int& n2, int& n1) {
  n4 = iters > kGuidedT4 ? (iters - kGuidedT4 + 3) >> 2 : 0;
  const int rem = iters - 4 * n4;                    // T4-3..T4, or iters itself when <= T4
  n2 = rem > kGuidedT2 ? (rem - kGuidedT2 + 1) >> 1 : 0;
  n1 = rem - 2 * n2;                                 // T2-1..T2 (0 only for iters == 0)
}
__host__ __device__ inline int me_num_tasks_guided(int wx, int wy) {
  const int quads = (wx + 3) >> 2;
  const int wy_low = me_fold(quads, wy) ? wy - 1 : wy;
  int n = 0;
  for (int k = 5; k >= 0; --k)
    if (quads & (1 << k)) {
      int n4, n2, n1;
      me_guided(((k == 5 ? wy : wy_low) + (64 >> k) - 1) / (64 >> k), n4, n2, n1);
      n += n4 + n2 + n1;
    }
  return n;
}

// 16-bit kernel: height of the strips a wx x wy window is cut into, given the most rows LDS holds (rows_max) and the number of
// strips the launch provides (max_strips).  The four waves of a workgroup pull lane-iterations from a counter and meet at a barrier
// after each column-parity pass, so a pass of n iterations costs ceil(n / 4) rounds: 25 iterations cost 7 rounds, 24 cost 6.
// Iterations of a pass over h rows: ceil(h * lanes_per_row / 64), lanes_per_row = ceil(candidates of one parity / 3) (three
// candidates per lane; the even pass has at least as many as the odd one).
// Strips are of EQUAL height ceil(wy / n): what a launch loses at its end is about half the lifetime of its longest workgroup, and
// a tall strip next to a short one made every launch measured slower than the even split of the same iterations (129 rows on
// 4 080 workgroups: 65 + 64 5.07 ms, 69 + 60 5.23, 81 + 48 6.10; 257 rows: 5 x 52 19.05 ms, 5 x 47 + 22 19.69).  The number of
// strips is the one with the fewest rounds, a strip counting half a round for its two window loads; ties go to fewer strips.
__host__ __device__ inline int me_strip_rows16(int wx, int wy, int rows_max, int max_strips) {
  const int lanes = (((wx + 1) >> 1) + 2) / 3;
  int best_h = (wy + max_strips - 1) / max_strips, best_cost = 0x7fffffff;
  for (int n = (wy + rows_max - 1) / rows_max; n <= max_strips && n <= wy; ++n) {
    const int h = (wy + n - 1) / n;
    const int used = (wy + h - 1) / h, rest = wy - (used - 1) * h;
    const int cost = 2 * ((used - 1) * ((((h * lanes + 63) >> 6) + 3) >> 2) + ((((rest * lanes + 63) >> 6) + 3) >> 2)) + used;
    if (cost < best_cost) { best_cost = cost; best_h = h; }
  }
  return best_h;
}

// The current picture is read from its CTU-BLOCKED copy (hmme_plane::d_blocks, written by me_fill_blocks_kernel beside the padded plane): CTU
// (cx, cy) is one contiguous block of 64 rows x 64 samples, blocks in raster order, partial edge CTUs completed by edge replication.  A
// current-block load of the search kernels is then `s_load_dwordx2 / x4` at the IMMEDIATE offset row * 64 * BPS + 8 * BPS * q from the block's
// address, whatever the picture's size: no pitch in the kernel, no s_mul_i32 in front of the 512 loads of a lane-iteration (5.5 % of its
// instructions -- round 5 removed them for the pitches of 2160p and 1080p planes only, by compile-time pitch instantiations that this
// layout replaces), the block's 64 (128) cache lines consecutive instead of one per plane row.  The per-CTU call hands over a dense
// 64 x 64 block already: one block, the same kernels.
constexpr int kBlkBytes8 = 64 * 64, kBlkBytes16 = 2 * 64 * 64;
// Pulls a workgroup's current block (64 * LINES consecutive 64-byte lines) into the scalar cache while the window is being staged:
// the first lane-iteration would otherwise meet every line cold, one CU at a time -- visible where a workgroup runs only a few
// iterations (the per-CTU call: 64 workgroups per search).  One wave issues the loads; nothing reads the results.
template <int LINES>
__device__ __forceinline__ void me_prefetch_cur(uint64_t curc) {
  // every load targets the SAME register `d`, an in-out operand of each statement and of the final wait: it stays allocated for the
  // whole sequence, so the compiler can never hand it to another value while loads into it are still in flight -- the inline scalar
  // loads are invisible to its own waitcnt / liveness tracking
  uint32_t d = 0;
#pragma unroll
  for (int l = 0; l < 64 * LINES; ++l) asm volatile("s_load_dword %0, %1, %2" : "+s"(d) : "s"(curc), "n"(64 * l));
  asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(d));
}

// Window staging shared by the search kernels: LDS dword i = window row i / PDW, dword i % PDW, realigned by `mis` bytes.  Eight
// loads are in flight per thread before the first one is waited for: the straightforward loop (load, wait, store) cost one memory
// round trip per 256 dwords -- 37 of them for a 129 x 129 window, ~4 % of a workgroup's lifetime, 63 per pass and strip (12 %) in
// the 16-bit kernel.
template <int PDW, int THREADS>
__device__ __forceinline__ void me_stage_window(uint32_t* win, const uint32_t* __restrict__ src_al, int pitch_dw, int n, uint32_t mis, int tid) {
  constexpr int U = 8;
  for (int i0 = tid; i0 < n; i0 += THREADS * U) {
    uint32_t lo[U], hi[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = min(i0 + u * THREADS, n - 1);          // clamped: every load is in bounds, surplus ones are not stored
      const int r = i / PDW, k = i - r * PDW;
      lo[u] = src_al[(long)r * pitch_dw + k];
      hi[u] = src_al[(long)r * pitch_dw + k + 1];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = i0 + u * THREADS;
      if (i < n) win[i] = __builtin_amdgcn_alignbyte(hi[u], lo[u], mis);
    }
  }
}

// Segment table of a SPLIT = 2 launch of me_search_kernel (written by me_prep_segments_kernel), one allocation:
//   int4    segs[W]        per workgroup: (job its segment starts in, first unit, end unit, h) in the list of UNITS of the launch's TAIL jobs
//                          (jobs h .. n - 1), or (job, 0, 0, -1): the workgroup searches that job whole (the head jobs 0 .. h - 1, one each)
//   MeJob16 jobs[n]        the jobs (y0 / y1 unused; `job` = index into the result arrays); me_finalize16_kernel decodes against them
//   int     prefix[n + 1]  entry j - h: units of the tail jobs before job j -- job j >= h owns the list's units [prefix[j - h], prefix[j - h + 1])
// Head and tail in ONE launch: the head's workgroups come first in the grid, and a segment starts on whichever slot a head job (the clipped
// windows of the picture's edge CTUs make short ones) leaves first -- as two launches the tail waited for the head's last workgroup.
// A unit is kSegUnit = 4 consecutive tasks (lane-iterations) of one job -- one per wave of the workgroup; a job's last unit may be short.
// Segments are cut at unit boundaries: where a segment leaves one job and enters the next the four waves meet at a barrier, and a piece
// of a job that is not a multiple of four tasks would leave waves idle in its last round on BOTH sides of every such boundary.
constexpr int kSegUnit = 4;
__host__ __device__ inline size_t me_seg_table_bytes(int n_wg, int n_jobs) { return sizeof(int4) * (size_t)n_wg + sizeof(MeJob16) * (size_t)n_jobs + sizeof(int) * ((size_t)n_jobs + 1); }
__host__ __device__ inline const int4* me_seg_table_segs(const void* t) { return (const int4*)t; }
__host__ __device__ inline const MeJob16* me_seg_table_jobs(const void* t, int n_wg) { return (const MeJob16*)((const int4*)t + n_wg); }
__host__ __device__ inline const int* me_seg_table_prefix(const void* t, int n_wg, int n_jobs) { return (const int*)(me_seg_table_jobs(t, n_wg) + n_jobs); }

// ---- the search kernel --------------------------------------------------------------------------
// windows wider or taller than 129 candidates (8-bit planes, search range 65..128) are cut into up to 2 x 2 tiles of at most
// 129 x 129: MeJob16::job carries the tile's (x, y) index in bits 30 and 29 above the output job index
constexpr int kTileStep = 129, kTileJobMask = 0x1fffffff;
// SPLIT = 0: one workgroup searches the whole window of jobs[blockIdx.x] (MeJob) and writes its 593 results.
// SPLIT = 1: jobs are MeJob16; the workgroup runs tasks [y0, y1) only and merges into g_best with 64-bit atomicMin
//            (decoded afterwards by me_finalize16_kernel) -- used where one CTU must fill many CUs.
// SPLIT = 2: the tasks of ALL jobs of the launch form one list (job after job), cut into gridDim.x equal SEGMENTS (me_prep_segments_kernel);
//            the workgroup runs segment blockIdx.x, which may end one job and begin the next (window staged again, table merged per job).
//            A launch that does not fill whole rounds of the chip's workgroup slots -- a small picture, the jobs beyond the last full
//            round of a larger one -- is dealt this way: every workgroup gets the same number of lane-iterations, whatever the number
//            of jobs and however the picture's edge clips their windows.  jobs_v: MeSegTable layout (below).
// n_seg_jobs: SPLIT = 2 only, the number of jobs the segment table covers
// curs: the CTU-blocked copies of the current pictures (above me_prefetch_cur), cur_ctus_x: CTUs per picture row (blocks per block row).
// PK = 1: the packed-minimum twin (ME_PKMIN above; every <FEN, SPLIT> has one).  Same results, fewer instructions per lane-iteration;
// only for launches that pass me_pk_gate.
// PK = 2 (FEN 1 only): the twin and the full-task twin in one kernel, one wave-uniform branch per task (me_task_full); only for
// launches that pass me_pk2_gate.
template <int FEN, int SPLIT, int PK>
__global__ void __launch_bounds__(kThreads, 2)
me_search_kernel(const RefSet curs, int cur_ctus_x, const RefSet refs, int ref_pitch,
                 const void* __restrict__ jobs_v, uint32_t lambda_q16, int16_t* __restrict__ out_mv,
                 uint32_t* __restrict__ out_sad, unsigned long long* __restrict__ g_best, int fair_prio, int n_seg_jobs) {
  __shared__ uint32_t win[kWinRowsMax * kPDW];
  __shared__ unsigned long long best64[kParts];
  __shared__ int task_ctr;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
#ifdef ME_SEARCH_T_TIMELINE   // timing-only build (results are overwritten): when each workgroup starts, has its window staged, runs dry, ends (100 MHz wall clock)
  const unsigned long long tl_start = wall_clock64();
#endif
  MeJob job;
  int t_first = 0, t_end = 0x7fffffff, out_job = blockIdx.x;
  unsigned long long tile_off = 0;   // SPLIT, tiled windows: (y, x) of this tile's first candidate in the CTU's whole window
  int seg_j = 0, seg_g = 0, seg_end = 0, seg_head = 0;   // SPLIT = 2: the job the segment is in, the next unit of the tail's list, the segment's end; the number of head jobs (-1: this workgroup searches job seg_j whole)
  if constexpr (SPLIT == 2) {
    const int4 sg = me_seg_table_segs(jobs_v)[blockIdx.x];
    seg_j = sg.x; seg_g = sg.y; seg_end = sg.z; seg_head = sg.w;
    if (seg_head >= 0 && seg_g >= seg_end) return;      // fewer units than workgroups (tiny windows): nothing for this one
  } else if constexpr (SPLIT == 1) {
    const MeJob16 jb = ((const MeJob16*)jobs_v)[blockIdx.x];
    job = jb.j; t_first = jb.y0; t_end = jb.y1; out_job = jb.job & kTileJobMask;
    tile_off = (unsigned long long)(((jb.job >> 29) & 1) * kTileStep) << 16 | (unsigned long long)(((jb.job >> 30) & 1) * kTileStep);
  } else {
    job = ((const MeJob*)jobs_v)[blockIdx.x];
    out_job = me_xcd_unit(blockIdx.x, gridDim.x);   // the job table of a whole-job launch is in XCD order (me_prep_jobs_kernel)
  }
  // every kernel argument and table entry loaded so far has arrived before the job loop: none of the compiler's own scalar loads stays
  // in flight into the loop's blocks, where tools/check_dpp_hazard.py (a linear scan) could not tell its wait from a missing one
  if constexpr (PK == 2) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll 1
  for (bool first_job = true;; first_job = false) {   // one pass, except SPLIT = 2: one pass per job the segment reaches into
  if constexpr (SPLIT == 2) {
    job = me_seg_table_jobs(jobs_v, gridDim.x)[seg_j].j;
    out_job = seg_j;
    if (seg_head >= 0) {
      const int* prefix = me_seg_table_prefix(jobs_v, gridDim.x, n_seg_jobs) - seg_head;
      const int p0 = prefix[seg_j], p1 = prefix[seg_j + 1];
      t_first = (seg_g - p0) * kSegUnit; t_end = (min(seg_end, p1) - p0) * kSegUnit;   // the job's last unit may be short: n_tasks clips
      seg_g = p1; ++seg_j;
    }                                  // else: a head job, whole (t_first = 0, t_end = everything; seg_g == seg_end: one pass)
    if (!first_job) __syncthreads();   // every thread has merged the previous job's table; window and table are free again
  }
  if (fair_prio) __builtin_amdgcn_s_setprio(3);   // a new workgroup comes first: its window loads go out at once, its first tasks run ahead of the older workgroup's last
  const uint8_t* __restrict__ ref_base = refs.base[job.ctu_x & 63];
  const uint8_t* __restrict__ cur_base = curs.base[job.ctu_x & 63];
  job.ctu_x &= ~63;
  const int wx = job.rb_x - job.lt_x + 1, wy = job.rb_y - job.lt_y + 1;   // candidates per row / rows

  for (int s = tid; s < kParts; s += kThreads) best64[s] = ~0ull;
  if (tid == 0) task_ctr = t_first;

  // -- 0. the current block is read through the scalar cache straight into SGPRs (v_qsad_pk_u16_u8 takes its 4 current-block bytes
  //       from one): no LDS copy, no wave-uniform ds_read_b64 (each cost a full LDS slot), 35 VGPRs fewer
  const uintptr_t cur_addr = (uintptr_t)(cur_base + ((long)(job.ctu_y >> 6) * cur_ctus_x + (job.ctu_x >> 6)) * kBlkBytes8);
  const uint64_t curc = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)cur_addr) |
                        (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(cur_addr >> 32)) << 32;
  if (tid < 64) me_prefetch_cur<1>(curc);
  // -- 1. stage the reference window: LDS row r, byte b  <->  ref(ctu_x + lt_x + b, ctu_y + lt_y + r)
  {
    const uint8_t* src = ref_base + (long)(job.ctu_y + job.lt_y) * ref_pitch + (job.ctu_x + job.lt_x);
    const uint32_t mis = (uint32_t)(uintptr_t)src & 3u;
    const uint32_t* src_al = (const uint32_t*)(src - mis);
    const int pitch_dw = ref_pitch >> 2;
    const int n = (wy + 63) * kPDW;
    me_stage_window<kPDW, kThreads>(win, src_al, pitch_dw, n, mis, tid);
  }
  __syncthreads();
#ifdef ME_SEARCH_T_TIMELINE
  const unsigned long long tl_staged = wall_clock64();
#endif

  // -- 2. task list: the ceil(wx/4) candidate quads of a row are split into power-of-two parts
  //       (129 -> 32 + 1); part k lays a wave out as 2^k quads x (64 >> k) rows per iteration.
  const int quads = (wx + 3) >> 2;
  constexpr int kIt = SPLIT ? kIterPerTaskSplit : kIterPerTask;
  constexpr bool kGuided = !SPLIT;
  const int n_tasks = kGuided ? me_num_tasks_guided(wx, wy) : min(me_num_tasks(wx, wy, kIt), t_end);
  const bool fold = me_fold(quads, wy);
  const int wy_low = fold ? wy - 1 : wy;

  const uint32_t mult_a = 1u << kIdxBits;
  const uint32_t mult_e = FEN ? (2u << kIdxBits) : (1u << kIdxBits);
  const bool rb1 = lane & 2, rb0 = lane & 1;
  // Wave priority falls with the wave's progress (s_setprio 3 .. 0 over its expected share of the workgroup's lane-iterations).  A SIMD
  // holds one wave of each of the CU's two workgroups and issues from the OLDER one whenever it can: of two workgroups that start
  // together the older ran at full speed and the younger in its gaps (a fifth of the rate), then alone -- one wave per SIMD issues at
  // ~0.8 of what two do -- for the rest of its life (profiles/r05b_search_timeline.txt: lifetimes 415 / 675 us in a single-round 1080p
  // launch).  With the wave that is behind given the SIMD first, the two stay within a quarter of their work of each other and end
  // together; in a launch of several rounds the same rule shortens the lonely ends of each CU's last workgroups.
  // state: lane-iterations left at the current level << 2 | level (0..3 = s_setprio 3..0); without priorities the first level never ends
  int prio_quarter = 0x0fffffff;
  if (fair_prio) {
    if constexpr (!SPLIT) {
      int total = 0;
      for (int kk = 5; kk >= 0; --kk)
        if (quads & (1 << kk)) total += ((kk == 5 ? wy : wy_low) + (64 >> kk) - 1) / (64 >> kk);
      prio_quarter = max(1, (total + 15) >> 4);   // a quarter of a wave's share (four waves)
    } else {
      prio_quarter = max(1, ((n_tasks - t_first) * kIt + 15) >> 4);   // this workgroup's slice of the CTU's tasks
    }
  }
  int prio_state = prio_quarter << 2;

  static_assert(SPLIT != 2 || kIterPerTaskSplit == 1, "segment mode counts tasks in lane-iterations");
  int grab_next = 0, grab_end = 0;   // SPLIT = 2: the tasks this wave has drawn and not yet run
  // running minima: register g, lane l <-> slot ME_SLOT_OF[g][l] (ME_SLOT_OF3 in a full task).  b0..b7 of a full task hold packed slots
  // only; a whole-job launch keeps them across the wave's full tasks of one part (kCarry: keys of me_carry_index, flushed before a task
  // that is not full or lies in another part, and when the counter runs dry).  carry_k >= 0: they hold minima of part (carry_k, carry_x0)
  constexpr bool kCarry = PK == 2 && SPLIT == 0;
  uint32_t b0 = ME_MAXKEY, b1 = ME_MAXKEY, b2 = ME_MAXKEY, b3 = ME_MAXKEY, b4 = ME_MAXKEY, b5 = ME_MAXKEY,
           b6 = ME_MAXKEY, b7 = ME_MAXKEY, b8 = ME_MAXKEY, b9 = ME_MAXKEY;
  int carry_k = -1, carry_x0 = 0;
  while (true) {
    int t = 0;
    if constexpr (SPLIT == 2) {
      // a wave draws a quarter of what is left, at most 4 tasks, and runs them as ONE task of that many lane-iterations where they lie in
      // one part of the window (one flush of the running minima for up to four lane-iterations instead of one each); guided
      // self-scheduling over the four waves ends them level: 12 tasks go 3 + 3 + 2 + 1, + 1 + 1 + 1 = three each
      if (grab_next >= grab_end) {
        int want = 0;
        if (lane == 0) {
          const int left = n_tasks - *(volatile int*)&task_ctr;
          want = min(4, max(1, (left + 3) >> 2));
          t = atomicAdd(&task_ctr, want);
        }
        t = __builtin_amdgcn_readfirstlane(t);
        want = __builtin_amdgcn_readfirstlane(want);
        if (t >= n_tasks) break;
        grab_next = t; grab_end = min(t + want, n_tasks);
      }
      t = grab_next;
    } else {
      if (lane == 0) t = atomicAdd(&task_ctr, 1);
      t = __builtin_amdgcn_readfirstlane(t);
      if (!kCarry && t >= n_tasks) break;   // kCarry: a dry counter decodes to no task at all (below), which flushes what is carried
    }
    const bool dry = t >= n_tasks;
    if (prio_state < 4 && (prio_state & 3) < 3) {   // the level's share is used up: one step down
      prio_state += (prio_quarter << 2) + 1;
      if ((prio_state & 3) == 1) __builtin_amdgcn_s_setprio(2);
      else if ((prio_state & 3) == 2) __builtin_amdgcn_s_setprio(1);
      else __builtin_amdgcn_s_setprio(0);
    }
    // decode task t -> (x0, k, first iteration)
    int x0 = 0, k = 0, it0 = 0, n_it = 0;
    {
      int xq = 0, rem = t;
      for (int kk = 5; kk >= 0; --kk) {
        if (!(quads & (1 << kk))) continue;
        const int iters = ((kk == 5 ? wy : wy_low) + (64 >> kk) - 1) / (64 >> kk);
        int nt;
        if constexpr (kGuided) {
          int n4, n2, n1;
          me_guided(iters, n4, n2, n1);
          nt = n4 + n2 + n1;
          if (rem < nt) {
            x0 = xq * 4; k = kk;
            if (rem < n4) { it0 = 4 * rem; n_it = 4; }
            else if (rem < n4 + n2) { it0 = 4 * n4 + 2 * (rem - n4); n_it = 2; }
            else { it0 = 4 * n4 + 2 * n2 + (rem - n4 - n2); n_it = 1; }
            break;
          }
        } else {
          nt = (iters + kIt - 1) / kIt;
          if (rem < nt) {
            x0 = xq * 4; k = kk; it0 = rem * kIt; n_it = min(kIt, iters - it0);
            if constexpr (SPLIT == 2) { n_it = min(grab_end - grab_next, iters - it0); grab_next += n_it; }   // kIt = 1: tasks are lane-iterations
            break;
          }
        }
        rem -= nt;
        xq += 1 << kk;
      }
    }
    const int ty = 64 >> k;
    const bool full = PK == 2 && me_task_full(wx, wy, k, it0, n_it);   // wave-uniform: wx, wy of the job, k, it0, n_it of the task
    const bool fold_part = fold && k == 5;

    if constexpr (kCarry) {
      // what the wave carries belongs to the full tasks of one part: anything else (no task at all included) sends it to the CTU table
      if (carry_k >= 0 && !(full && k == carry_k && x0 == carry_x0)) {
#define ME_FLUSH_CARRIED(g, key_)                                                                                  \
        {                                                                                                          \
          const int slot = ME_SLOT_OF3[g][lane];                                                                   \
          const uint32_t key = (key_);                                                                             \
          const uint32_t cost = key >> kIdxBits;                                                                   \
          if (slot >= 0 && cost < kInvCost) {                                                                      \
            int row, group;                                                                                        \
            me_carry_position(carry_k, key & ((1u << kIdxBits) - 1), row, group);                                  \
            atomicMin(&best64[slot], ((unsigned long long)cost << 32) | ((unsigned long long)row << 16) |          \
                                         (unsigned long long)(carry_x0 + 16 * group));                             \
          }                                                                                                        \
        }
        ME_FLUSH_CARRIED(0, b0) ME_FLUSH_CARRIED(1, b1) ME_FLUSH_CARRIED(2, b2) ME_FLUSH_CARRIED(3, b3)
        ME_FLUSH_CARRIED(4, b4) ME_FLUSH_CARRIED(5, b5) ME_FLUSH_CARRIED(6, b6) ME_FLUSH_CARRIED(7, b7)
#undef ME_FLUSH_CARRIED
        carry_k = -1;
      }
      if (dry) break;
    }
    if (carry_k < 0) b0 = b1 = b2 = b3 = b4 = b5 = b6 = b7 = ME_MAXKEY;
    b8 = b9 = ME_MAXKEY;

    // A full task's lanes all lie inside the window, on the same columns in every lane-iteration: the x halves of its four MV costs
    // (me_component_bits <= 37 each, one byte apiece), the key's lane field and the window address of its first lane-iteration are
    // the task's, and a lane-iteration adds what its rows change (the prologue of the full-task body below)
    uint32_t f_bx = 0, f_tag = 0;
    int f_vy = 0;
    const lds_char_t* f_lpc = (const lds_char_t*)win;
    if (full) {
      // the lane's quad and row inside a lane-iteration: a full task puts the two lowest bits of the quad index into lane bits 5 and 4
      // (four adjacent quads in lanes l, l ^ 16, l ^ 32, l ^ 48: the two packed butterfly levels), the rest and ly into bits 0..3
      const int lx = ((lane >> 5) & 1) | ((lane >> 3) & 2) | ((lane & ((1 << (k - 2)) - 1)) << 2), ly = (lane & 15) >> (k - 2);
      const int cx = x0 + 4 * lx, cy = it0 * ty + ly;
      const int vx = ((job.lt_x + cx) << 2) - job.pred_x;
      f_bx = me_component_bits(vx) | me_component_bits(vx + 4) << 8 | me_component_bits(vx + 8) << 16 | me_component_bits(vx + 12) << 24;
      f_tag = (uint32_t)(ly << k | lx) << 2;   // the key's lane field: raster order inside the lane-iteration
      f_vy = ((job.lt_y + cy) << 2) - job.pred_y;
      f_lpc = (const lds_char_t*)(win + cy * kPDW + (cx >> 2));
    }
    // scalar loads complete out of order: ME8_CUR_WAIT (placed by the generator one CU after the loads, before the next CU's are
    // issued) waits for the batch; the window dwords of the same batch are named first so that the compiler's LDS wait lands there
#define ME8_CUR(row, q)                                                                                                            \
  ({                                                                                                                               \
    uint64_t w_;                                                                                                                   \
    asm volatile("s_load_dwordx2 %0, %1, %2" : "=s"(w_) : "s"(curc), "n"((row) * 64 + 8 * (q)));                                    \
    w_;                                                                                                                            \
  })
#define ME8_CUR_WAIT(w0, w1, w2, w3, w4, w5, w6, w7, d0, d1, d2, d3, d4, d5, d6, d7, d8, d9, d10, d11, d12, d13, d14, d15)           \
  asm volatile("" : : "v"(d0), "v"(d1), "v"(d2), "v"(d3), "v"(d4), "v"(d5), "v"(d6), "v"(d7), "v"(d8), "v"(d9), "v"(d10), "v"(d11),  \
               "v"(d12), "v"(d13), "v"(d14), "v"(d15));                                                                             \
  asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(w0), "+s"(w1), "+s"(w2), "+s"(w3), "+s"(w4), "+s"(w5), "+s"(w6), "+s"(w7))

    prio_state -= n_it << 2;
    for (int it = 0; it < n_it; ++it) {
      if (full) {
        if constexpr (PK == 2) {
          static_assert(PK != 2 || FEN == 1, "the full-task body exists for FEN 1");
          // every lane valid with all four candidates: no validity selects, no marker, no clamps.  me_pk2_gate bounds the products
          // below 2^32 and the costs, their high halves, below 2^16: a byte permute packs two of them
          const uint32_t by = me_component_bits_xad(f_vy + it * (4 * ty));
          const uint32_t p0 = lambda_q16 * ((f_bx & 255u) + by), p1 = lambda_q16 * (((f_bx >> 8) & 255u) + by);
          const uint32_t p2 = lambda_q16 * (((f_bx >> 16) & 255u) + by), p3 = lambda_q16 * ((f_bx >> 24) + by);
          const uint64_t pkm = (uint64_t)__builtin_amdgcn_perm(p1, p0, 0x07060302u) | (uint64_t)__builtin_amdgcn_perm(p3, p2, 0x07060302u) << 32;
          // the 64-bit negation of pkm (the strips that leave a 16x16 region as sums give the costs back with one add of it: no field
          // borrows, each holds at least its cost) as complement + 1: one 64-bit add where 0 - pkm is a borrow pair; opaque on both sides,
          // or the compiler folds it back, and turns the body's add of a negation into a 64-bit subtract
          uint64_t npkm = ~pkm;
          asm volatile("" : "+v"(npkm));
          npkm += 1;
          asm volatile("" : "+v"(npkm));
          const uint32_t tag = ((uint32_t)it << 8) | f_tag;
          // the key constant of the packed slots names the 16-candidate group (its first quad): per task, or per part where carried
          const uint32_t ctag = kCarry ? (uint32_t)(it0 + it) << kCarryGroupBits | f_tag >> 4 : tag & ~(3u << 2);
          const uint32_t c0 = (p0 >> 16) << kIdxBits | tag, c1 = (p1 >> 16) << kIdxBits | tag | 1u;
          const uint32_t c2 = (p2 >> 16) << kIdxBits | tag | 2u, c3 = (p3 >> 16) << kIdxBits | tag | 3u;
          const uint32_t nc0 = me_neg_xad(c0), nc1 = me_neg_xad(c1), nc2 = me_neg_xad(c2), nc3 = me_neg_xad(c3);
          const lds_char_t* lpc = f_lpc + it * (ty * kPDW * 4);
#include "me_tree_pk4_fen1.inc"
        }
        continue;
      }
      // the key's lane field, raster order inside the lane-iteration, is the lane itself here: quad lx of row ly.  Opaque, so that neither
      // they nor `lane << 2` join the loop-invariant registers, which the full-task body would have to carry (at 255 VGPRs the one value spilled)
      uint32_t lane_now = (uint32_t)lane;
      asm("" : "+v"(lane_now));
      const int lx = lane_now & ((1 << k) - 1), ly = lane_now >> k;
      int cx = x0 + 4 * lx, cy = (it0 + it) * ty + ly;
      if (fold_part && cy == wy) { cx += 128; cy = wy - 1; }   // idle second row of the last iteration: leftover quads of the last row
      const bool vy = cy < wy;
      // per-candidate constants: (mv cost | invalid marker) << 10 | iteration | lane | j
      const int mvy = job.lt_y + cy, mvx = job.lt_x + cx;
      const uint32_t by = me_component_bits((mvy << 2) - job.pred_y);
      const uint32_t tag = ((uint32_t)it << 8) | (lane_now << 2);
      uint32_t cc[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t cost = (lambda_q16 * (me_component_bits(((mvx + j) << 2) - job.pred_x) + by)) >> 16;
        cc[j] = (((vy && (cx + j) < wx) ? cost : kInvCost) << kIdxBits) | tag | (uint32_t)j;
      }
      const uint32_t c0 = cc[0], c1 = cc[1], c2 = cc[2], c3 = cc[3];
      const uint32_t nc0 = 0u - c0, nc1 = 0u - c1, nc2 = 0u - c2, nc3 = 0u - c3;
      // PK: the same four MV costs as packed u16 (the gate keeps them below kPkMarker - kPkSlotMax), and the lane's key constant
      uint64_t pkm = 0;
      uint32_t ctag = 0;
      if constexpr (PK) {
        const uint32_t m0 = cc[0] < (kInvCost << kIdxBits) ? cc[0] >> kIdxBits : kPkMarker, m1 = cc[1] < (kInvCost << kIdxBits) ? cc[1] >> kIdxBits : kPkMarker;
        const uint32_t m2 = cc[2] < (kInvCost << kIdxBits) ? cc[2] >> kIdxBits : kPkMarker, m3 = cc[3] < (kInvCost << kIdxBits) ? cc[3] >> kIdxBits : kPkMarker;
        pkm = (uint64_t)(m0 | m1 << 16) | (uint64_t)(m2 | m3 << 16) << 32;
        ctag = ((vy && cx < wx) ? 0u : kInvCost << kIdxBits) | tag;   // candidate 0 is valid wherever one of the four is
      }
      // lanes outside the window still run (wave-uniform code) on clamped, in-bounds addresses
      const lds_char_t* lpc = (const lds_char_t*)(win + min(cy, wy - 1) * kPDW + (min(cx, wx - 1) >> 2));
      if constexpr (PK == 2) {
#include "me_tree_pk_fen1.inc"
      } else if constexpr (PK) {
        if constexpr (FEN) {
#include "me_tree_pk_fen1.inc"
        } else {
#include "me_tree_pk_fen0.inc"
        }
      } else if constexpr (FEN) {
#include "me_tree_fen1.inc"
      } else {
#include "me_tree_fen0.inc"
      }
    }

    // -- 3. fold the wave's running minima into the CTU table; (cost, y, x) keys give raster-order ties
#define ME_FLUSH(g, key_)                                                                                          \
    {                                                                                                              \
      const int slot = full ? ME_SLOT_OF3[g][lane] : ME_SLOT_OF[g][lane];                                          \
      const uint32_t key = (key_);                                                                                 \
      const uint32_t cost = key >> kIdxBits;                                                                       \
      if (slot >= 0 && cost < kInvCost) {                                                                          \
        const int kit = (key >> 8) & 3, kl = (key >> 2) & 63, kj = key & 3;                                        \
        int bx = x0 + 4 * (kl & ((1 << k) - 1)) + kj;                                                              \
        int byy = (it0 + kit) * ty + (kl >> k);                                                                    \
        if (fold_part && byy == wy) { bx += 128; byy = wy - 1; }                                                   \
        atomicMin(&best64[slot],                                                                                   \
                  ((unsigned long long)cost << 32) | ((unsigned long long)byy << 16) | (unsigned long long)bx);    \
      }                                                                                                            \
    }
    if (!(kCarry && full)) {
      ME_FLUSH(0, b0) ME_FLUSH(1, b1) ME_FLUSH(2, b2) ME_FLUSH(3, b3)
      ME_FLUSH(4, b4) ME_FLUSH(5, b5) ME_FLUSH(6, b6) ME_FLUSH(7, b7)
    } else {      // the packed minima of a full task stay with the wave (above)
      carry_k = k; carry_x0 = x0;
    }
    ME_FLUSH(8, b8) ME_FLUSH(9, b9)
#undef ME_FLUSH
  }
#ifdef ME_SEARCH_T_TIMELINE
  const unsigned long long tl_dry = wall_clock64();   // this wave found the task counter dry
#endif
  __syncthreads();
#ifdef ME_SEARCH_T_TIMELINE
  const unsigned long long tl_all = wall_clock64();
#endif

  // -- 4. results: integer MV (TComMv layout) and the pure SAD at the arg-min (ruiSAD, reference
  //       TEncSearch.cpp:3895: best - getCost(best))
  if constexpr (SPLIT) {
    for (int s = tid; s < kParts; s += kThreads) {
      unsigned long long v = best64[s];
      if constexpr (PK) v = me_pk_recover<PK == 2>(v, s, win, kPDW, (const uint8_t*)cur_addr, job, wx, lambda_q16);   // before the entry leaves the workgroup
      if (v != ~0ull) atomicMin(&g_best[(long)out_job * kParts + s], v + tile_off);
    }
    if constexpr (SPLIT == 2) {
      if (seg_g < seg_end) continue;   // the segment goes on in the next job
    }
    return;
  }
  for (int s = tid; s < kParts; s += kThreads) {
    unsigned long long v = best64[s];
    if constexpr (PK) v = me_pk_recover<PK == 2>(v, s, win, kPDW, (const uint8_t*)cur_addr, job, wx, lambda_q16);
    const int mvx = job.lt_x + (int)(v & 0xffff), mvy = job.lt_y + (int)((v >> 16) & 0xffff);
    const uint32_t cost = (uint32_t)(v >> 32);
    const long o = (long)out_job * kParts + s;
    out_mv[2 * o] = (int16_t)mvx;
    out_mv[2 * o + 1] = (int16_t)mvy;
    out_sad[o] = cost - me_mv_cost(lambda_q16, mvx, mvy, job.pred_x, job.pred_y);
  }
#ifdef ME_SEARCH_T_TIMELINE
  __syncthreads();
  if (lane == 0) {
    uint32_t* o = out_sad + (long)out_job * kParts;
    const int wv = tid >> 6;
    if (wv == 0) {
      const unsigned long long t1 = wall_clock64();
      uint32_t hw_id;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));
      uint32_t xcc_id;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_id));
      o[0] = (uint32_t)tl_start; o[1] = (uint32_t)(tl_start >> 32); o[2] = (uint32_t)(tl_staged - tl_start); o[3] = (uint32_t)(tl_all - tl_start);
      o[4] = (uint32_t)(t1 - tl_start); o[5] = hw_id; o[6] = xcc_id; o[7] = blockIdx.x;
    }
    o[8 + wv] = (uint32_t)(tl_dry - tl_start);
  }
#endif
  break;   // SPLIT = 0: the one job is done (SPLIT = 1 returned above, SPLIT = 2 went on or returned)
  }
}

// ---- frame helpers ---------------------------------------------------------------------------------

// TComDataCU::clipMv (reference TComDataCU.cpp:2907-2920), quarter pels, maxCU = 64
__host__ __device__ inline void clip_mv_q(int& x, int& y, int cu_x, int cu_y, int pic_w, int pic_h) {
  const int hor_max = (pic_w + 8 - cu_x - 1) << 2, hor_min = (-64 - 8 - cu_x + 1) << 2;
  const int ver_max = (pic_h + 8 - cu_y - 1) << 2, ver_min = (-64 - 8 - cu_y + 1) << 2;
  x = (int16_t)(x > hor_max ? hor_max : (x < hor_min ? hor_min : x));
  y = (int16_t)(y > ver_max ? ver_max : (y < ver_min ? ver_min : y));
}
// TEncSearch::xSetSearchRange (reference TEncSearch.cpp:3814-3830)
__host__ __device__ inline void set_search_range(int pred_x, int pred_y, int sr, int cu_x, int cu_y, int pic_w,
                                                 int pic_h, int& lt_x, int& lt_y, int& rb_x, int& rb_y) {
  int px = pred_x, py = pred_y;
  clip_mv_q(px, py, cu_x, cu_y, pic_w, pic_h);
  int ltx = (int16_t)(px - (sr << 2)), lty = (int16_t)(py - (sr << 2));
  int rbx = (int16_t)(px + (sr << 2)), rby = (int16_t)(py + (sr << 2));
  clip_mv_q(ltx, lty, cu_x, cu_y, pic_w, pic_h);
  clip_mv_q(rbx, rby, cu_x, cu_y, pic_w, pic_h);
  lt_x = ltx >> 2; lt_y = lty >> 2; rb_x = rbx >> 2; rb_y = rby >> 2;
}

// The MeJob of job i of a launch over CTUs [ctu_first, ctu_first + ctu_count) of a picture and its references: reference r = i / ctu_count
// (packed into the low six bits of ctu_x, whose CTU origins are multiples of 64), CTU ctu_first + i % ctu_count.  pred_q and center_q are
// [n_refs][CTUs of the picture][2], quarter pels.  Null pred_q: zero predictors.  center_q: the window's centre where it is not the
// predictor -- HM's bi-prediction pass searches around the list's current MV and prices MV bits against the AMVP predictor
// (TEncSearch.cpp:3726-3737); null: the predictor.  Every job table and the table-less refinement launch take their jobs from here.
__host__ __device__ __forceinline__ MeJob me_picture_job(int i, const int16_t* __restrict__ pred_q, const int16_t* __restrict__ center_q,
                                                         int ctu_first, int ctu_count, int pic_w, int pic_h, int sr) {
  const int r = i / ctu_count;
  const int ctus_x = (pic_w + 63) >> 6, n_ctu = ctus_x * ((pic_h + 63) >> 6);
  const int ctu = ctu_first + (i - r * ctu_count);
  const int cu_x = (ctu % ctus_x) * 64, cu_y = (ctu / ctus_x) * 64;
  const long pq = 2 * ((long)r * n_ctu + ctu);
  const int px = pred_q ? pred_q[pq] : 0, py = pred_q ? pred_q[pq + 1] : 0;
  const int wx_q = center_q ? center_q[pq] : px, wy_q = center_q ? center_q[pq + 1] : py;
  int ltx, lty, rbx, rby;
  set_search_range(wx_q, wy_q, sr, cu_x, cu_y, pic_w, pic_h, ltx, lty, rbx, rby);
  MeJob j;
  j.ctu_x = (int16_t)(cu_x | r); j.ctu_y = (int16_t)cu_y;
  j.lt_x = (int16_t)ltx; j.lt_y = (int16_t)lty; j.rb_x = (int16_t)rbx; j.rb_y = (int16_t)rby;
  j.pred_x = (int16_t)px; j.pred_y = (int16_t)py;
  return j;
}
// tile (tx, ty) of a window beyond 129 x 129 candidates: the sub-window of step kTileStep, clipped to the job's right-bottom
__host__ __device__ inline MeJob me_tile_job(MeJob job, int tx, int ty) {
  const int x1 = job.lt_x + (tx + 1) * kTileStep - 1, y1 = job.lt_y + (ty + 1) * kTileStep - 1;
  job.lt_x = (int16_t)(job.lt_x + tx * kTileStep); job.lt_y = (int16_t)(job.lt_y + ty * kTileStep);
  job.rb_x = (int16_t)(x1 < job.rb_x ? x1 : job.rb_x); job.rb_y = (int16_t)(y1 < job.rb_y ? y1 : job.rb_y);
  return job;
}

// one MeJob per (CTU, reference) search: jobs [job0, job0 + n_jobs) of the launch (me_picture_job); jobs[] is indexed from job0
// xcd_order: jobs[] is written in the XCD-aware order of me_search_kernel<FEN, 0> (position li holds job job0 + me_xcd_unit(li, n_jobs));
// 0 for the refinement kernel, which takes job blockIdx.x
// job_counter (may be null): the refinement kernel's work counter, reset here for the launch that follows on the same stream
__global__ void me_prep_jobs_kernel(MeJob* jobs, const int16_t* __restrict__ pred_q, int ctu_first, int ctu_count,
                                    int n_refs, int pic_w, int pic_h, int sr, int job0, int n_jobs, int xcd_order, uint32_t* job_counter,
                                    const int16_t* __restrict__ center_q) {
  const int li = blockIdx.x * blockDim.x + threadIdx.x;
  if (li == 0 && job_counter) *job_counter = 0;
  if (li >= n_jobs) return;
  const int i = job0 + (xcd_order ? me_xcd_unit(li, n_jobs) : li);
  jobs[li] = me_picture_job(i, pred_q, center_q, ctu_first, ctu_count, pic_w, pic_h, sr);
}

// picture area (int16 Pel, u16 or u8; pitch in elements) -> padded u8 / u16 plane, borders edge-replicated like
// TComPicYuv::extendPicBorder (reference TComPicYuv.cpp:214-262).  One thread per 4 output bytes.
// flag[0] is set when a sample lies outside [0, max_val].
template <typename SrcT, typename DstT>
__global__ void me_fill_plane_kernel(uint8_t* __restrict__ dst, int dst_pitch, int margin_x, int margin_y, int w, int h,
                                     const SrcT* __restrict__ src, int src_pitch, int max_val, int* __restrict__ flag) {
  constexpr int N = 4 / (int)sizeof(DstT);                        // samples per thread
  const int x0 = (blockIdx.x * blockDim.x + threadIdx.x) * N;   // plane column of the first sample
  const int y = blockIdx.y;                                       // plane row
  if (x0 * (int)sizeof(DstT) >= dst_pitch) return;
  const int sy = min(max(y - margin_y, 0), h - 1);
  uint32_t packed = 0;
  bool bad = false;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int sx = min(max(x0 + i - margin_x, 0), w - 1);
    const int v = (int)src[(long)sy * src_pitch + sx];
    bad |= (v < 0) | (v > max_val);
    packed |= (uint32_t)(v & (sizeof(DstT) == 1 ? 0xff : 0xffff)) << (8 * (int)sizeof(DstT) * i);
  }
  *(uint32_t*)(dst + (long)y * dst_pitch + (long)x0 * sizeof(DstT)) = packed;
  if (bad) atomicOr(flag, 1);
}

// the same picture area -> the plane's CTU-blocked copy (see me_prefetch_cur): block (cx, cy) holds samples (64 cx + c, 64 cy + r) at
// [r][c], coordinates beyond the picture clamped to its last column / row (what the padded plane holds there).  One thread per 4 output
// bytes, a row of a block per 16 (32) threads: 64-byte (128-byte) contiguous writes.  Range violations are the padded fill's to report.
template <typename SrcT, typename DstT>
__global__ void me_fill_blocks_kernel(uint8_t* __restrict__ dst, int ctus_x, int n_ctu, int w, int h, const SrcT* __restrict__ src, int src_pitch) {
  constexpr int N = 4 / (int)sizeof(DstT);                        // samples per thread
  constexpr int PER_ROW = 64 / N, PER_BLK = 64 * PER_ROW;         // threads per block row / per block
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int blk = (int)(t / PER_BLK), in = (int)(t - (long)blk * PER_BLK);
  if (blk >= n_ctu) return;
  const int r = in / PER_ROW, c0 = (in - r * PER_ROW) * N;
  const int sy = min((blk / ctus_x) * 64 + r, h - 1), x0 = (blk % ctus_x) * 64 + c0;
  uint32_t packed = 0;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int v = (int)src[(long)sy * src_pitch + min(x0 + i, w - 1)];
    packed |= (uint32_t)(v & (sizeof(DstT) == 1 ? 0xff : 0xffff)) << (8 * (int)sizeof(DstT) * i);
  }
  *(uint32_t*)(dst + t * 4) = packed;
}

// ---- 16-bit sample path (bit depth 9..12, bi-prediction origins of any depth) -----------------------------------------------
// Same task / key / butterfly / merge machinery as me_search_kernel; differences (see tools/gen_me_tree.py, class Tree16):
// v_sad_u16 leaves on u16 samples, three candidates per lane (x, x+2, x+4), exact 32-bit sums (candidates 0 and 1 as one 64-bit
// register pair: one add for both) and
//   key = ((sum << fen_shift) >> (bitDepth-8)) << kIdxBits16 + c     (reference TComRdCost.cpp:520-521)
// formed as (S' & ~0xff) + c from sums that the tree's first add of two leaves has already shifted to the key's field,
// lanes packed linearly over the window (candidate triple q = iteration*64 + lane), one lane-iteration per task, and the window
// is cut into horizontal strips of candidate rows so that one strip's reference rows fit LDS (SR 128: 320 x 322 samples); strips
// of a CTU are separate workgroups that merge through 64-bit atomicMin on a global table.
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef volatile __attribute__((address_space(3))) uint32_t lds_vu32_t;
typedef volatile __attribute__((address_space(3))) u32x4_t lds_vu32x4_t;
#define ME_SAD16(a, b, acc) __builtin_amdgcn_sad_u16((a), (b), (acc))

// key of each of the lane's three candidates from its exact sum, and their minimum; `asm volatile` for the same reason as me_min4
// (ordered against the masked merges).  The sums arrive shifted to the key's sum field (the tree's first add of two leaf sums shifts
// the result, tools/gen_me_tree.py Tree16): key = (S' & ~0xff) + c -- the mask drops the bits HM's >> (bitDepth-8) drops.
// This three-register form is what the generator emits with PAIR64 = False (the A/B build); the kernel as shipped uses me_keymin3_p
__device__ __forceinline__ uint32_t me_keymin3(uint32_t s0, uint32_t s1, uint32_t s2, uint32_t mask, uint32_t c0, uint32_t c1, uint32_t c2) {
  uint32_t r, t, u;
  asm volatile("v_and_b32 %0, %6, %3\n\tv_and_b32 %1, %6, %4\n\tv_and_b32 %2, %6, %5\n\t"
               "v_add_u32 %0, %0, %7\n\tv_add_u32 %1, %1, %8\n\tv_add_u32 %2, %2, %9\n\t"
               "v_min3_u32 %0, %0, %1, %2"
               : "=&v"(r), "=&v"(t), "=&v"(u) : "v"(s0), "v"(s1), "v"(s2), "s"(mask), "v"(c0), "v"(c1), "v"(c2));
  return r;
}

#define ME16_KEYMIN(s0, s1, s2) me_keymin3(s0, s1, s2, keymask16, c0, c1, c2)
// the same with candidates 0 and 1 as one 64-bit pair (tools/gen_me_tree.py PAIR64): two v_and_b32 on its halves, ONE 64-bit add for both
// keys (v_lshl_add_u64, shift 0; neither half carries into the other: a key is below 2^32), and + add for the third, v_min3_u32 -- six
// instructions where three separate candidates took seven.  Only the minimum is `asm volatile` (ordered against the masked merges)
__device__ __forceinline__ uint64_t me_pair(uint32_t lo, uint32_t hi) { return (uint64_t)lo | (uint64_t)hi << 32; }
__device__ __forceinline__ uint32_t me_keymin3_p(uint64_t s01, uint32_t s2, uint32_t mask, uint64_t c01, uint32_t c2) {
  const uint64_t k01 = (s01 & me_pair(mask, mask)) + c01;
  const uint32_t k2 = (s2 & mask) + c2;
  uint32_t r;
  asm volatile("v_min3_u32 %0, %1, %2, %3" : "=v"(r) : "v"((uint32_t)k01), "v"((uint32_t)(k01 >> 32)), "v"(k2));
  return r;
}
#define ME16_KEYMIN_P(s01, s2) me_keymin3_p(s01, s2, keymask16, c01, c2)

#ifdef ME_SEARCH_T_TIMELINE   // timing-only builds: per workgroup of me_search16_kernel -- start, [per pass: window staged, wave 0 dry, all dry], end (100 MHz wall clock), hardware id
__device__ uint32_t g_timeline16[16384 * 12];
#endif
// curs / cur_ctus_x: the CTU-blocked copies of the current pictures (u16 samples: 8 KiB per block), as in me_search_kernel
template <int FEN, int PDW>
__global__ void __launch_bounds__(kThreads16, 2)
me_search16_kernel(const RefSet curs, int cur_ctus_x, const RefSet refs, int ref_pitch,
                   const MeJob16* __restrict__ jobs, uint32_t lambda_q16, int sh, unsigned long long* __restrict__ g_best, int fair_prio) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  unsigned long long* best64 = (unsigned long long*)smem;              // [593] (+1 pad)
  int* task_ctr = (int*)(smem + 2 * 594);
  uint32_t* win = smem + 2 * 594 + 4;                                  // [(ny + 63)][PDW]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  if (fair_prio) __builtin_amdgcn_s_setprio(3);   // wave priority falls with the wave's progress: me_search_kernel
#ifdef ME_SEARCH_T_TIMELINE
  const unsigned long long tl0 = wall_clock64();
  uint32_t tl[8];
  int tln = 0;
#define ME16_STAMP() tl[tln++] = (uint32_t)(wall_clock64() - tl0)
#else
#define ME16_STAMP()
#endif
  const MeJob16 jb = jobs[blockIdx.x];
  MeJob job = jb.j;
  const uint8_t* __restrict__ ref_base = refs.base[job.ctu_x & 63];
  const uint8_t* __restrict__ cur_base = curs.base[job.ctu_x & 63];
  job.ctu_x &= ~63;
  const int wx = job.rb_x - job.lt_x + 1;
  const int ny = jb.y1 - jb.y0;                                        // candidate rows of this strip

  for (int s = tid; s < kParts; s += kThreads16) best64[s] = ~0ull;
  // key = ((sum << lsh) & ~0xff) + c  ==  (((sum << fen_shift) >> sh) << kIdxBits16) + c; the shift rides on the tree's first adds
  const uint32_t lsh_a = kIdxBits16 - sh, lsh_e = FEN ? kIdxBits16 + 1 - sh : lsh_a;
  const uint32_t keymask16 = ~((1u << kIdxBits16) - 1u);
  const bool rb1 = lane & 2, rb0 = lane & 1;
  constexpr int ME16_PDW = PDW;
  // The current block comes through the scalar cache into SGPRs (v_sad_u16 takes one SGPR operand): no LDS slot and no VGPR for
  // it -- as a wave-uniform ds_read_b128 each of its 512 reads per lane-iteration cost a full LDS slot, a third of the kernel's LDS
  // time.  Scalar loads complete out of order: ME16_CUR_WAIT (placed by the generator half a CU after the loads, before the next
  // batch is issued) waits for the whole batch and ties the loaded quads to the wait; the window dwords of the same batch are
  // named as inputs so that the compiler's own LDS wait lands in front of it, not behind the next batch.
  const uintptr_t cur_addr = (uintptr_t)(cur_base + ((long)(job.ctu_y >> 6) * cur_ctus_x + (job.ctu_x >> 6)) * kBlkBytes16);
  const uint64_t curc = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)cur_addr) |
                        (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(cur_addr >> 32)) << 32;
  if (tid < 64) me_prefetch_cur<2>(curc);
#define ME16_CUR(row, q)                                                                                                           \
  ({                                                                                                                               \
    u32x4_t w_;                                                                                                                    \
    asm volatile("s_load_dwordx4 %0, %1, %2" : "=s"(w_) : "s"(curc), "n"((row) * 128 + 16 * (q)));                                  \
    w_;                                                                                                                            \
  })
#define ME16_CUR_WAIT(w0, w1, w2, w3, d0, d1, d2, d3, d4, d5, d6, d7, d8, d9, d10, d11)                                               \
  asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(w0), "+s"(w1), "+s"(w2), "+s"(w3)                                                       \
               : "v"(d0), "v"(d1), "v"(d2), "v"(d3), "v"(d4), "v"(d5), "v"(d6), "v"(d7), "v"(d8), "v"(d9), "v"(d10), "v"(d11))

  // Two passes: the even window columns, then the odd ones, each over a window loaded with a shift of `par` samples.
  // A lane owns the candidates (x, x + 2, x + 4): all read dword-aligned u16 pairs, each one dword further on -- the six dwords
  // three 64-bit reads of a window row deliver.  Lane bases are 3 dwords apart: 4-byte-aligned reads (ds_read2_b32).
#pragma unroll 1
  for (int par = 0; par < 2; ++par) {
    if (par) __syncthreads();                                          // every wave is done with the previous window
    if (tid == 0) *task_ctr = 0;
    {
      const uint8_t* src = ref_base + (long)(job.ctu_y + job.lt_y + jb.y0) * ref_pitch + 2 * (job.ctu_x + job.lt_x + par);
      const uint32_t mis = (uint32_t)(uintptr_t)src & 3u;
      const uint32_t* src_al = (const uint32_t*)(src - mis);
      const int pitch_dw = ref_pitch >> 2;
      const int n = (ny + 63) * PDW;
      me_stage_window<PDW, kThreads16>(win, src_al, pitch_dw, n, mis, tid);
    }
    __syncthreads();
    ME16_STAMP();

  const int n_par = (wx + 1 - par) >> 1;                               // candidates of this column parity per window row
  const int pairs = (n_par + 2) / 3;                                   // lanes per window row
  const int n_iters = (ny * pairs + 63) >> 6;
  const int n_tasks = n_iters;                                         // one lane-iteration per task: a pass is ~25 iterations for 4 waves

  while (true) {
    int t = 0;
    if (lane == 0) t = atomicAdd(task_ctr, 1);
    t = __builtin_amdgcn_readfirstlane(t);
    if (t >= n_tasks) break;
    const int it0 = t;
    constexpr int n_it = 1;
    // Priority by the WORKGROUP's progress (the pass and the half of its iterations the task counter has reached), the same for its
    // four waves: they meet at a barrier after each pass, and per-wave levels (me_search_kernel's scheme) let the wave that had pulled
    // one iteration more fall behind the others by another -- barrier waits of 100 us instead of 35 (profiles/r05q_search16_timeline.txt)
    if (fair_prio) {
      const int lvl = 2 * par + (2 * t >= n_tasks ? 1 : 0);
      if (lvl == 0) __builtin_amdgcn_s_setprio(3);
      else if (lvl == 1) __builtin_amdgcn_s_setprio(2);
      else if (lvl == 2) __builtin_amdgcn_s_setprio(1);
      else __builtin_amdgcn_s_setprio(0);
    }
    uint32_t b0 = ME_MAXKEY, b1 = ME_MAXKEY, b2 = ME_MAXKEY, b3 = ME_MAXKEY, b4 = ME_MAXKEY, b5 = ME_MAXKEY,
             b6 = ME_MAXKEY, b7 = ME_MAXKEY, b8 = ME_MAXKEY, b9 = ME_MAXKEY;
    for (int it = 0; it < n_it; ++it) {
      const int q = (it0 + it) * 64 + lane;
      const int row = q / pairs, pr = q - row * pairs;
      const int cx = par + 6 * pr, cy = jb.y0 + row;
      const bool vy = row < ny;
      const int mvy = job.lt_y + cy, mvx = job.lt_x + cx;
      const uint32_t by = me_component_bits((mvy << 2) - job.pred_y);
      const uint32_t tag = (uint32_t)lane << 2;
      uint32_t cc[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const uint32_t cost = (lambda_q16 * (me_component_bits(((mvx + 2 * j) << 2) - job.pred_x) + by)) >> 16;
        cc[j] = (((vy && (cx + 2 * j) < wx) ? cost : kInvCost16) << kIdxBits16) | tag | (uint32_t)j;
      }
      const uint32_t c0 = cc[0], c1 = cc[1], c2 = cc[2];
      const uint64_t c01 = me_pair(c0, c1);
      const lds_char_t* lpd = (const lds_char_t*)(win + min(row, ny - 1) * PDW + 3 * pr);
      if constexpr (FEN) {
#include "me_tree16_fen1.inc"
      } else {
#include "me_tree16_fen0.inc"
      }
    }
    // where a winning candidate lies: the key names the lane that owned it, and that lane knows its row and first column -- one
    // ds_bpermute_b32 (all lanes active here) instead of a division by `pairs` per running-minimum register (ten per task; the task
    // is one lane-iteration of this kernel, and its time follows its instruction count)
    const uint32_t my_yx = [&] {
      const int q = it0 * 64 + lane, row = q / pairs;
      return (uint32_t)(jb.y0 + row) << 16 | (uint32_t)(par + 6 * (q - row * pairs));
    }();
#define ME_FLUSH16(g, key_)                                                                                        \
    {                                                                                                              \
      const int slot = ME_SLOT_OF[g][lane];                                                                        \
      const uint32_t key = (key_);                                                                                 \
      const uint32_t cost = key >> kIdxBits16;                                                                     \
      const uint32_t yx = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(key & 0xfcu), (int)my_yx);   /* lane (key >> 2) & 63, in bytes */ \
      if (slot >= 0 && cost < kInvCost16)                                                                          \
        atomicMin(&best64[slot], ((unsigned long long)cost << 32) | (unsigned long long)(yx + 2 * (key & 3)));     \
    }
    ME_FLUSH16(0, b0) ME_FLUSH16(1, b1) ME_FLUSH16(2, b2) ME_FLUSH16(3, b3) ME_FLUSH16(4, b4)
    ME_FLUSH16(5, b5) ME_FLUSH16(6, b6) ME_FLUSH16(7, b7) ME_FLUSH16(8, b8) ME_FLUSH16(9, b9)
#undef ME_FLUSH16
  }
    ME16_STAMP();   // this wave found the pass's counter dry
#ifdef ME_SEARCH_T_TIMELINE
    __syncthreads();
    ME16_STAMP();   // all waves dry
#endif
  }   // par
#undef ME16_CUR
#undef ME16_CUR_WAIT
  __syncthreads();
  for (int s = tid; s < kParts; s += kThreads16) atomicMin(&g_best[(long)jb.job * kParts + s], best64[s]);
#ifdef ME_SEARCH_T_TIMELINE
  if (tid == 0 && blockIdx.x < 16384) {
    uint32_t* o = g_timeline16 + blockIdx.x * 12;
    uint32_t hw_id;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));
    o[0] = (uint32_t)tl0; o[1] = (uint32_t)(tl0 >> 32);
    for (int i = 0; i < 6; ++i) o[2 + i] = tl[i];
    o[8] = (uint32_t)(wall_clock64() - tl0); o[9] = hw_id; o[10] = (uint32_t)ny; o[11] = (uint32_t)wx;
  }
#endif
#undef ME16_STAMP
}

// strips of one CTU have merged into g_best: decode (cost, y, x) -> TComMv + pure SAD.  Every entry read is set back to all ones: the
// table is left as the next launch needs it (hmme.hip merge_table: no preset launch in front of every split / strip / segment launch)
__global__ void me_finalize16_kernel(unsigned long long* __restrict__ g_best, const MeJob16* __restrict__ jobs,
                                     const int* __restrict__ first_strip_of_job, int n_jobs, uint32_t lambda_q16,
                                     int16_t* __restrict__ out_mv, uint32_t* __restrict__ out_sad) {
  const long o = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= (long)n_jobs * kParts) return;
  const MeJob job = jobs[first_strip_of_job[o / kParts]].j;
  const unsigned long long v = g_best[o];
  g_best[o] = ~0ull;
  const int mvx = job.lt_x + (int)(v & 0xffff), mvy = job.lt_y + (int)((v >> 16) & 0xffff);
  out_mv[2 * o] = (int16_t)mvx;
  out_mv[2 * o + 1] = (int16_t)mvy;
  out_sad[o] = (uint32_t)(v >> 32) - me_mv_cost(lambda_q16, mvx, mvy, job.pred_x, job.pred_y);
}

// one MeJob16 per (CTU, strip) from the per-CTU predictors
// ---- per-CTU call: everything stays on the compute queue ------------------------------------------------------------
// the call block (jobs, merge-table preset, current block, window) is pulled from mapped pinned host memory by the GPU itself
// -- no copy-engine hop and no cross-queue dependency in front of the search kernel
__global__ void me_stage_call_kernel(const uint4* __restrict__ host_block, uint4* __restrict__ dev_block, int n16) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n16) dev_block[i] = host_block[i];
}
// explicit weighted prediction (TEncSearch::setWpScalingDistParam, TEncSearch.cpp:5594-5635): the search of a slice with weighted
// prediction prices |org - (((w0 * ref + round) >> shift) + offset)| (TComRdCostWeightPrediction::xGetSADw,
// TComRdCostWeightPrediction.cpp:79-81).  The prediction of a sample does not depend on the candidate, so the staged window of a
// per-CTU call is weighted ONCE, into a second buffer (u16 samples, `bias` added so that block and window stay unsigned), and the 16-bit search
// kernel runs on it unchanged.
__global__ void me_weight_window_kernel(const uint8_t* __restrict__ win, uint8_t* __restrict__ out, int pitch, int rows, int cols, int w0, int round,
                                        int shift, int offset_bias) {
  // eight samples past the last one of each row are written too, as zeros: the search kernel stages whole 16-byte pieces past the last sample,
  // and what it finds there must be defined like the raw window's padding (hmme.hip ctu_call) -- `out` is never cleared otherwise
  const int i = blockIdx.x * blockDim.x + threadIdx.x, cw = cols + 8;
  if (i >= rows * cw) return;
  const int y = i / cw, x = i - y * cw;
  if (x >= cols) { ((uint16_t*)(out + (long)y * pitch))[x] = 0; return; }
  const uint16_t v = ((const uint16_t*)(win + (long)y * pitch))[x];
  ((uint16_t*)(out + (long)y * pitch))[x] = (uint16_t)(((w0 * (int)v + round) >> shift) + offset_bias);   // the raw window stays: the refinement interpolates IT
}

// read-and-clear of a latched range-violation flag in one step: a fill kernel on another stream that sets it concurrently is either
// seen by this take or by the next one, never lost between a read and a separate clear
__global__ void me_take_flag_kernel(int* flag, int* out) { *out = atomicExch(flag, 0); }

// single-job finalize (one workgroup) that writes the results straight into mapped pinned host memory and then publishes a
// sequence number there: the host polls that word instead of sleeping in hipStreamSynchronize
__global__ void __launch_bounds__(640)
me_finalize1_kernel(const unsigned long long* __restrict__ g_best, const MeJob16* __restrict__ jobs, uint32_t lambda_q16,
                    int16_t* __restrict__ out_mv, uint32_t* __restrict__ out_sad, volatile uint32_t* done_flag, uint32_t seq) {
  const int o = threadIdx.x;
  if (o < kParts) {
    const MeJob job = jobs[0].j;
    const unsigned long long v = g_best[o];
    const int mvx = job.lt_x + (int)(v & 0xffff), mvy = job.lt_y + (int)((v >> 16) & 0xffff);
    out_mv[2 * o] = (int16_t)mvx;
    out_mv[2 * o + 1] = (int16_t)mvy;
    out_sad[o] = (uint32_t)(v >> 32) - me_mv_cost(lambda_q16, mvx, mvy, job.pred_x, job.pred_y);
  }
  __threadfence_system();
  __syncthreads();
  if (o == 0) { *done_flag = seq; __threadfence_system(); }
}

// completion word of a per-CTU call whose last kernel is not the finalize kernel (search + refinement)
__global__ void me_publish_kernel(volatile uint32_t* done_flag, uint32_t seq) {
  __threadfence_system();
  *done_flag = seq;
  __threadfence_system();
}

// jobs [0, tail_first) are cut into n_strips strips, jobs from tail_first on into tail_strips (the last, partial round of
// workgroups of a launch is dealt in finer pieces, hmme.hip plan_tail)
__global__ void me_prep_jobs16_kernel(MeJob16* jobs, int* first_strip_of_job, const int16_t* __restrict__ pred_q,
                                      int ctu_first, int ctu_count, int n_refs, int pic_w, int pic_h, int sr, int n_strips_head, int rows_max,
                                      int tail_first, int tail_strips, const int16_t* __restrict__ center_q) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ctu_count * n_refs) return;
  const MeJob j = me_picture_job(i, pred_q, center_q, ctu_first, ctu_count, pic_w, pic_h, sr);
  const int wx = j.rb_x - j.lt_x + 1, wy = j.rb_y - j.lt_y + 1;
  const int n_strips = i < tail_first ? n_strips_head : tail_strips;
  const int base = i < tail_first ? i * n_strips_head : tail_first * n_strips_head + (i - tail_first) * tail_strips;
  const int n_units = tail_first * n_strips_head + (ctu_count * n_refs - tail_first) * tail_strips;   // workgroups of the launch
  first_strip_of_job[i] = me_xcd_position(base, n_units);
  // strips of the height me_strip_rows16 picks for this window, the last one takes the rest; strips beyond the window (clipped
  // windows need fewer) are empty: y0 == y1
  // head jobs: the planner's choice within n_strips; tail jobs: exactly tail_strips equal pieces (the host chose that number for
  // the sake of the launch's last round, not for this window)
  const int h = i < tail_first ? me_strip_rows16(wx, wy, rows_max, n_strips) : max(1, (wy + n_strips - 1) / n_strips);
  for (int s = 0; s < n_strips; ++s) {
    MeJob16 js;
    js.j = j;
    js.y0 = (int16_t)min(wy, s * h);
    js.y1 = (int16_t)min(wy, (s + 1) * h);
    js.job = i;
    // XCD-aware order (me_xcd_position): the strips of a CTU, whose window rows overlap by 63, and the CTUs next to it run on ONE
    // XCD, one after the other; every XCD gets all strips of its CTUs, so strips of unequal height cannot pile up on one XCD (round 2
    // rotated the strip order per job for that)
    jobs[me_xcd_position(base + s, n_units)] = js;
  }
}

// 8-bit segment mode (me_search_kernel SPLIT = 2): the jobs' units (kSegUnit tasks) as one list, cut into n_wg equal segments.  ONE workgroup of
// kSegPrepThreads threads writes the whole table (n_jobs <= kSegPrepThreads: a tail is shorter than one round of the chip's workgroup slots):
// a job and its unit count per thread, an inclusive scan in LDS, then the segments -- segment s owns units [N s / n_wg, N (s + 1) / n_wg)
// and starts in the job whose range holds its first unit (binary search in the prefix sums).
constexpr int kSegPrepThreads = 512;
// the head of a segment launch: jobs 0 .. n_head - 1, one workgroup each, in the XCD-aware order of a whole-job launch (me_xcd_unit)
__global__ void me_prep_whole_segments_kernel(void* table, int* first_strip_of_job, const int16_t* __restrict__ pred_q, int ctu_first, int ctu_count,
                                              int n_refs, int pic_w, int pic_h, int sr, int n_wg, int n_head) {
  const int li = blockIdx.x * blockDim.x + threadIdx.x;
  if (li >= n_head) return;
  MeJob16 js;
  js.j = me_picture_job(li, pred_q, nullptr, ctu_first, ctu_count, pic_w, pic_h, sr);
  js.y0 = 0; js.y1 = 0x7fff; js.job = li;
  ((MeJob16*)me_seg_table_jobs(table, n_wg))[li] = js;
  first_strip_of_job[li] = li;
  ((int4*)me_seg_table_segs(table))[me_xcd_position(li, n_head)] = make_int4(li, 0, 0, -1);
}
// the tail: the launch's jobs job0 .. job0 + n_jobs - 1 as entries idx0 .. of the table's jobs and as its segments idx0 .. n_wg - 1.
// idx0 = job0: the head's jobs are entries / workgroups 0 .. job0 - 1 of the same table (one launch); idx0 = 0: a table of the tail alone
__global__ void __launch_bounds__(kSegPrepThreads)
me_prep_segments_kernel(void* table, int* first_strip_of_job, const int16_t* __restrict__ pred_q, int ctu_first, int ctu_count, int n_refs,
                        int pic_w, int pic_h, int sr, int n_wg, int job0, int n_jobs, int idx0) {
  __shared__ int scan[kSegPrepThreads + 1];
  const int li = threadIdx.x;
  int nt = 0;
  if (li < n_jobs) {
    const int i = job0 + li;              // which (CTU, reference): the launch's job i
    MeJob16 js;
    js.j = me_picture_job(i, pred_q, nullptr, ctu_first, ctu_count, pic_w, pic_h, sr);
    nt = me_num_tasks(js.j.rb_x - js.j.lt_x + 1, js.j.rb_y - js.j.lt_y + 1);
    js.y0 = 0; js.y1 = (int16_t)nt; js.job = idx0 + li;
    nt = (nt + kSegUnit - 1) / kSegUnit;   // from here on: units
    ((MeJob16*)me_seg_table_jobs(table, n_wg))[idx0 + li] = js;
    first_strip_of_job[idx0 + li] = idx0 + li;   // me_finalize16_kernel: entry e decodes against jobs[e]
  }
  scan[li + 1] = nt;
  if (li == 0) scan[0] = 0;
  __syncthreads();
  for (int d = 1; d < kSegPrepThreads; d <<= 1) {   // inclusive scan over scan[1 ..]
    const int v = li + 1 > d ? scan[li + 1 - d] : 0;
    __syncthreads();
    scan[li + 1] += v;
    __syncthreads();
  }
  int* prefix = (int*)me_seg_table_prefix(table, n_wg, idx0 + n_jobs);
  if (li <= n_jobs) prefix[li] = scan[li];
  const long total = scan[n_jobs];
  int4* segs = (int4*)me_seg_table_segs(table) + idx0;
  const int n_seg = n_wg - idx0;
  for (int s = li; s < n_seg; s += kSegPrepThreads) {
    const int g0 = (int)(total * s / n_seg), g1 = (int)(total * (s + 1) / n_seg);
    int lo = 0, hi = n_jobs;                         // the job j with scan[j] <= g0 < scan[j + 1] (every job has at least one task)
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (scan[mid] <= g0) lo = mid; else hi = mid;
    }
    segs[s] = make_int4(idx0 + lo, g0, g1, idx0);
  }
}

// 8-bit planes, search range 65..128: four tile jobs per (CTU, reference), each a complete search of its sub-window through the
// SPLIT kernel; tile (0,0) comes first and keeps the window's own top-left, which me_finalize16_kernel decodes against
__global__ void me_prep_jobs_tile_kernel(MeJob16* jobs, int* first_strip_of_job, const int16_t* __restrict__ pred_q,
                                         int ctu_first, int ctu_count, int n_refs, int pic_w, int pic_h, int sr) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ctu_count * n_refs) return;
  const MeJob j = me_picture_job(i, pred_q, nullptr, ctu_first, ctu_count, pic_w, pic_h, sr);
  first_strip_of_job[i] = i * 4;
  for (int t = 0; t < 4; ++t) {
    const int tx = t & 1, ty = t >> 1;
    const bool empty = j.lt_x + tx * kTileStep > j.rb_x || j.lt_y + ty * kTileStep > j.rb_y;
    MeJob16 js;
    js.j = empty ? me_tile_job(j, 0, 0) : me_tile_job(j, tx, ty);   // a tile the clipped window does not reach keeps the window's own top-left
    js.y0 = 0; js.y1 = empty ? 0 : 0x7fff;   // task range: everything, or nothing for a tile the clipped window does not reach
    js.job = i | tx << 30 | ty << 29;
    jobs[i * 4 + t] = js;
  }
}


// ---- fractional-pel refinement of the integer winners ---------------------------------------------------------
// The step after the path: TEncSearch::xPatternSearchFracDIF (reference TEncSearch.cpp:4294-4331) for all 593
// slots of a CTU -- half-pel then quarter-pel refinement around each slot's integer MV with HM's 8-tap luma
// interpolation (TComInterpolationFilter.cpp:57-63, :170-260) and Hadamard (xGetHADs, TComRdCost.cpp:1537-1604)
// or SAD distortion.  Work item = one 4x4 block of one DISTINCT (position, MV) pair of the CTU ("Work sharing" below: at most 6 144
// per CTU and stage, far fewer where slots share their motion); one lane per item.  An 8x8 Hadamard is assembled from the four 4x4
// transforms of its quadrants (H8 = [[H4, H4], [H4, -H4]]) with two quad_perm DPP butterflies, so slots whose size is a multiple of 8
// (8x8 Hadamard blocks) and the others (4x4 blocks) run the same code.  Per-slot distortions accumulate in LDS (ds_add_u32); 593
// threads then add the MV cost and pick the winner in HM's point order (strict '<', tables TEncSearch.cpp:51-75).
// per-slot distortion sums of the nine refinement points
// BPS = bytes per sample of the planes (1: 8-bit video, 2: 9..12 bit)
// 8-bit planes: the nine sums of a slot are three 64-bit words of three 21-bit fields each (points 3k, 3k + 1, 3k + 2 of word k), added
// with ds_add_u64 -- a third of the LDS atomics, which on content whose slots share their motion were 40 % of an item's time (up to sixteen
// lanes of a wave add to the same large slot: profiles/r05k_frac_phases_before_after.txt).  A field never carries into the next: the largest sum is the
// 64x64 slot's, 64 8x8 Hadamard blocks of at most 8 * 64 * 255 / 4 = 32 640 each (Parseval) = 2 088 960 < 2^21; SAD 64 * 64 * 255.
// The bound is reached: a difference of +-255 in the sign pattern of the Sylvester matrix H8 (a bent function: all 64 coefficients 8 * 255)
// gives exactly 32 640 per 8x8 block, and tests/test_gpu_refine_spectral.py pins it (tests/spectral_content.py has the pictures).
// Wider samples (and the biased ones of bi-prediction origins) keep nine 32-bit sums.
constexpr bool frac_pack3(int bps) { return bps == 1; }
constexpr int frac_acc_row(int bps) { return frac_pack3(bps) ? 6 : 9; }   // dwords per slot
constexpr int frac_acc_dw(int bps) { return (593 * frac_acc_row(bps) + 15) & ~15; }
static_assert(64 * 32640 < (1 << 21) && 4096 * 255 < (1 << 21), "me_frac_kernel: a packed sum field holds the largest 8-bit slot sum");
constexpr int frac_threads(int bps) { return 256; }
// sums [593][9] | slot states | tap tables, counters | the two work lists | current block | cover table (uint16 [64][18] + [256][6])
constexpr size_t frac_lds_bytes(int bps) { return (size_t)(frac_acc_dw(bps) + 600 + 160 + (64 * 18 + 256 * 6) / 2 + 1024 * bps + (64 * 18 + 256 * 6) / 2) * 4; }

__device__ __forceinline__ uint32_t me_mv_cost_q(uint32_t lambda_q16, int vx_q, int vy_q, int pred_x, int pred_y) {
  return (lambda_q16 * (me_component_bits(vx_q - pred_x) + me_component_bits(vy_q - pred_y))) >> 16;
}

// luma taps of fraction f (0..3), tap t (0..7): TComInterpolationFilter::m_lumaFilter
__host__ __device__ constexpr int me_luma_tap(int f, int t) {
  constexpr int k1[8] = {-1, 4, -10, 58, 17, -5, 1, 0}, k2[8] = {-1, 4, -11, 40, 40, -11, 4, -1}, k3[8] = {0, 1, -5, 17, 58, -10, 4, -1};
  const int k0 = t == 3 ? 64 : 0;
  return f == 0 ? k0 : (f == 1 ? k1[t] : (f == 2 ? k2[t] : k3[t]));
}
// the 8 taps of quarter position q (-3..3, relative to the integer MV) as a 9-tap window that starts one sample
// earlier when the integer part of q is -1: tap j (0..8) multiplies patch sample (output column + j)
__host__ __device__ constexpr int me_tap9(int q, int j) {
  const int t = j - ((q >> 2) + 1);
  return (t < 0 || t > 7) ? 0 : me_luma_tap(q & 3, t);
}
// horizontal taps packed for the dot-product instructions: dword k of the tap window of output column c over the
// 12-sample patch row (BPS 1: four i8 per dword, v_dot4c_i32_i8; BPS 2: two i16 per dword, v_dot2c_i32_i16)
template <int BPS>
__host__ __device__ constexpr uint32_t me_htap_dw(int q, int c, int k) {
  uint32_t w = 0;
  for (int i = 0; i < 4 / BPS; ++i) {
    const int j = (4 / BPS) * k + i - c;
    const int t = (j < 0 || j > 8) ? 0 : me_tap9(q, j);
    w |= BPS == 1 ? (uint32_t)(t & 0xff) << (8 * i) : (uint32_t)(t & 0xffff) << (16 * i);
  }
  return w;
}
// Quarter-pel stage: the three offsets of a component around its half-pel winner h (-1, 0, +1 half samples) all fit ONE 8-sample
// window: h = -1 -> q = -3..-1, integer part -1: samples -4..+3; h = 0 -> q = -1..1: samples -3..+4 (q = -1 is fraction 3 at integer
// part -1, whose first tap is 0, so its seven live taps start at sample -3 as well); h = +1 -> q = 1..3: samples -3..+4.  The lane
// fetches its patch from that window's first sample on -- 11 x 11 samples instead of 12 x 12, 8 taps instead of a 9-tap window with a
// zero at one end.  me_tap8(h3, d3, j): tap of window sample j (0..7) for winner h3 - 1 and offset d3 - 1 (both 0..2).
__host__ __device__ constexpr int me_win8_first(int h3) { return h3 == 0 ? -4 : -3; }   // first window sample relative to the output sample
__host__ __device__ constexpr int me_tap8(int h3, int d3, int j) {
  const int q = 2 * (h3 - 1) + (d3 - 1);
  const int t = j + me_win8_first(h3) - ((q >> 2) - 3);   // tap index: sample = out + (q >> 2) - 3 + t
  return (t < 0 || t > 7) ? 0 : me_luma_tap(q & 3, t);
}
static_assert(me_luma_tap(3, 0) == 0, "the tap q = -1 loses to the shared window must be zero");
// dword k of the packed 8-tap window (BPS 1: four i8 per dword; BPS 2: two i16)
template <int BPS>
__host__ __device__ constexpr uint32_t me_htap8_dw(int h3, int d3, int k) {
  uint32_t w = 0;
  for (int i = 0; i < 4 / BPS; ++i) {
    const int j = (4 / BPS) * k + i;
    const int t = j < 8 ? me_tap8(h3, d3, j) : 0;
    w |= BPS == 1 ? (uint32_t)(t & 0xff) << (8 * i) : (uint32_t)(t & 0xffff) << (16 * i);
  }
  return w;
}
constexpr int kFracTabH = 8, kFracTabV = 8;   // LDS tap tables: 9 rows (winner x offset) of packed horizontal / float vertical taps
constexpr int kFracRows1 = 11;                // patch rows (and samples per row) of the quarter-pel stage

#define ME_FRAC_BFLY(R, T, PERM) "v_fmac_f32_dpp " #R ", " #R ", " #T " quad_perm:" PERM " row_mask:0xf bank_mask:0xf\n\t"
__device__ __forceinline__ float me_dpp_f(float v, const int ctrl_b1) {
  return ctrl_b1 ? __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xf, 0xf, false))
                 : __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xf, 0xf, false));
}

// max(|a|, |b|) in ONE instruction: fmaxf() of two fabsf() compiles to three (llvm.maxnum quiets signalling NaNs first: a
// v_max_f32 x, |x|, |x| per operand in IEEE mode); no NaN ever reaches these
__device__ __forceinline__ float me_absmax(float a, float b) {
  float r;
  asm("v_max_f32 %0, |%1|, |%2|" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// distortion of one 4x4 difference block d (row-major): SAD, or the Hadamard sum (xCalcHADs4x4; with KIND8 the quad's four 4x4
// transforms are combined into the 8x8 transform, xCalcHADs8x8, and all four lanes return the block's value)
// want4 (wave-uniform, KIND8 only): also return in `own4` what this lane's 4x4 block alone contributes to a slot made of 4x4 blocks
// (the AMP shapes, 8x4, 4x8) -- the same difference block, the same 4x4 transform, only the 8x8 combination left out
template <int HAD, int KIND8>
__device__ __forceinline__ uint32_t me_frac_dist(const float (&d)[16], float s1, float s2, bool want4, uint32_t& own4) {
  uint32_t contrib;
  if (!HAD) {
    float sad = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) sad += __builtin_fabsf(d[i]);
    if (KIND8) {   // the quad's four 4x4 SADs belong to the same slots: hand out their sum
      own4 = (uint32_t)sad;
      sad += me_dpp_f(sad, 1);
      sad += me_dpp_f(sad, 0);
    }
    contrib = (uint32_t)sad;
  } else {
    float m[16];
#pragma unroll
    for (int r = 0; r < 4; ++r) {   // 4x4 Walsh-Hadamard: rows, then columns (xCalcHADs4x4)
      const float a = d[4 * r] + d[4 * r + 3], b = d[4 * r + 1] + d[4 * r + 2], e = d[4 * r + 1] - d[4 * r + 2], f = d[4 * r] - d[4 * r + 3];
      m[4 * r] = a + b; m[4 * r + 1] = a - b; m[4 * r + 2] = f + e; m[4 * r + 3] = f - e;
    }
    // columns, first level; z = {a, b, e, f}[k].  The second level would be a + b, a - b, f + e, f - e -- but only the sum of the
    // absolute coefficients is wanted and |a + b| + |a - b| = 2 max(|a|, |b|): the level and its sixteen absolute adds become eight
    // v_max_f32 (|.| is a source modifier) and eight adds of HALF the sum.  The levels of a Walsh-Hadamard transform commute, so with
    // KIND8 the two levels across the quad run BEFORE that last one -- and the lane's own 4x4 sum (want4) is the same eight maxima
    // taken before them.
    float z[16];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      z[k] = m[k] + m[12 + k]; z[4 + k] = m[4 + k] + m[8 + k]; z[8 + k] = m[4 + k] - m[8 + k]; z[12 + k] = m[k] - m[12 + k];
    }
    float sum = 0.f;
    if (KIND8) {   // combine the quad's four 4x4 transforms into the 8x8 transform (xCalcHADs8x8)
      if (want4) {   // xCalcHADs4x4 of this block, as the 4x4 kind computes it: ((2 * s4) + 1) >> 1
        float s4 = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) { const float t = me_absmax(z[k], z[4 + k]) + me_absmax(z[8 + k], z[12 + k]); s4 = k ? s4 + t : t; }
        own4 = (uint32_t)s4;
      }
      // two butterflies across the quad, each one v_fmac_f32 with a DPP source: z += t * z[neighbour], t = +-1 by
      // role.  Odd roles hold the negated difference, which the absolute sum does not see.  One asm block keeps
      // 16 instructions between a register's write and its DPP read (the hazard the assembler does not pad for).
      asm("s_nop 1\n\t"
          ME_FRAC_BFLY(%0, %16, "[1,0,3,2]") ME_FRAC_BFLY(%1, %16, "[1,0,3,2]") ME_FRAC_BFLY(%2, %16, "[1,0,3,2]") ME_FRAC_BFLY(%3, %16, "[1,0,3,2]")
          ME_FRAC_BFLY(%4, %16, "[1,0,3,2]") ME_FRAC_BFLY(%5, %16, "[1,0,3,2]") ME_FRAC_BFLY(%6, %16, "[1,0,3,2]") ME_FRAC_BFLY(%7, %16, "[1,0,3,2]")
          ME_FRAC_BFLY(%8, %16, "[1,0,3,2]") ME_FRAC_BFLY(%9, %16, "[1,0,3,2]") ME_FRAC_BFLY(%10, %16, "[1,0,3,2]") ME_FRAC_BFLY(%11, %16, "[1,0,3,2]")
          ME_FRAC_BFLY(%12, %16, "[1,0,3,2]") ME_FRAC_BFLY(%13, %16, "[1,0,3,2]") ME_FRAC_BFLY(%14, %16, "[1,0,3,2]") ME_FRAC_BFLY(%15, %16, "[1,0,3,2]")
          ME_FRAC_BFLY(%0, %17, "[2,3,0,1]") ME_FRAC_BFLY(%1, %17, "[2,3,0,1]") ME_FRAC_BFLY(%2, %17, "[2,3,0,1]") ME_FRAC_BFLY(%3, %17, "[2,3,0,1]")
          ME_FRAC_BFLY(%4, %17, "[2,3,0,1]") ME_FRAC_BFLY(%5, %17, "[2,3,0,1]") ME_FRAC_BFLY(%6, %17, "[2,3,0,1]") ME_FRAC_BFLY(%7, %17, "[2,3,0,1]")
          ME_FRAC_BFLY(%8, %17, "[2,3,0,1]") ME_FRAC_BFLY(%9, %17, "[2,3,0,1]") ME_FRAC_BFLY(%10, %17, "[2,3,0,1]") ME_FRAC_BFLY(%11, %17, "[2,3,0,1]")
          ME_FRAC_BFLY(%12, %17, "[2,3,0,1]") ME_FRAC_BFLY(%13, %17, "[2,3,0,1]") ME_FRAC_BFLY(%14, %17, "[2,3,0,1]") ME_FRAC_BFLY(%15, %17, "[2,3,0,1]")
          : "+v"(z[0]), "+v"(z[1]), "+v"(z[2]), "+v"(z[3]), "+v"(z[4]), "+v"(z[5]), "+v"(z[6]), "+v"(z[7]), "+v"(z[8]), "+v"(z[9]),
            "+v"(z[10]), "+v"(z[11]), "+v"(z[12]), "+v"(z[13]), "+v"(z[14]), "+v"(z[15])
          : "v"(s1), "v"(s2));
#pragma unroll
      for (int k = 0; k < 4; ++k) { const float t = me_absmax(z[k], z[4 + k]) + me_absmax(z[8 + k], z[12 + k]); sum = k ? sum + t : t; }
      sum += sum;
      sum += me_dpp_f(sum, 1);
      sum += me_dpp_f(sum, 0);
      contrib = ((uint32_t)sum + 2) >> 2;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) { const float t = me_absmax(z[k], z[4 + k]) + me_absmax(z[8 + k], z[12 + k]); sum = k ? sum + t : t; }
      contrib = (uint32_t)sum;   // (2 * sum + 1) >> 1
    }
  }
  return contrib;
}

// The Hadamard sum of a 4x4 difference block that arrives as pairs of horizontal neighbours (P[r][h]: row r, columns 2h, 2h + 1), two
// butterflies per instruction (v_pk_add_f32).  Only the sum of the absolute coefficients is wanted, so the transform runs in natural
// (Sylvester) order -- the same sixteen Walsh functions as xCalcHADs4x4's, in another order and with other signs: three levels pair
// different registers element by element, the one level that pairs the two halves of a register comes last, in scalar code (measured
// against the same level first: 2 % slower; and against this function in the half-pel stage, whose differences are born as single
// registers: 4 % slower, profiles/r04s_frac_instruction_mix_ab.txt).  The 8x8 combination across the quad works on corresponding
// coefficients of the four quadrants, which every lane orders alike.
typedef float v2f __attribute__((ext_vector_type(2)));
template <int KIND8>
__device__ __forceinline__ uint32_t me_frac_had_pk(const v2f (&P)[4][2], float s1, float s2, bool want4, uint32_t& own4) {
  v2f A[4][2], B[4][2], C[4][2];
#pragma unroll
  for (int r = 0; r < 4; ++r) { A[r][0] = P[r][0] + P[r][1]; A[r][1] = P[r][0] - P[r][1]; }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    B[0][h] = A[0][h] + A[1][h]; B[1][h] = A[0][h] - A[1][h]; B[2][h] = A[2][h] + A[3][h]; B[3][h] = A[2][h] - A[3][h];
    C[0][h] = B[0][h] + B[2][h]; C[2][h] = B[0][h] - B[2][h]; C[1][h] = B[1][h] + B[3][h]; C[3][h] = B[1][h] - B[3][h];
  }
  // the level that pairs the two halves of a register comes last and is never carried out: |x + y| + |x - y| = 2 max(|x|, |y|)
  // (me_frac_dist); with KIND8 the two levels across the quad run before it, the lane's own 4x4 sum is taken before those
  float z[16];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int h = 0; h < 2; ++h) { z[4 * r + 2 * h] = C[r][h].x; z[4 * r + 2 * h + 1] = C[r][h].y; }
  float sum = 0.f;
  if (KIND8) {
    if (want4) {
      float s4 = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) { const float t = me_absmax(z[2 * i], z[2 * i + 1]); s4 = i ? s4 + t : t; }
      own4 = (uint32_t)s4;
    }
    asm("s_nop 1\n\t"
        ME_FRAC_BFLY(%0, %16, "[1,0,3,2]") ME_FRAC_BFLY(%1, %16, "[1,0,3,2]") ME_FRAC_BFLY(%2, %16, "[1,0,3,2]") ME_FRAC_BFLY(%3, %16, "[1,0,3,2]")
        ME_FRAC_BFLY(%4, %16, "[1,0,3,2]") ME_FRAC_BFLY(%5, %16, "[1,0,3,2]") ME_FRAC_BFLY(%6, %16, "[1,0,3,2]") ME_FRAC_BFLY(%7, %16, "[1,0,3,2]")
        ME_FRAC_BFLY(%8, %16, "[1,0,3,2]") ME_FRAC_BFLY(%9, %16, "[1,0,3,2]") ME_FRAC_BFLY(%10, %16, "[1,0,3,2]") ME_FRAC_BFLY(%11, %16, "[1,0,3,2]")
        ME_FRAC_BFLY(%12, %16, "[1,0,3,2]") ME_FRAC_BFLY(%13, %16, "[1,0,3,2]") ME_FRAC_BFLY(%14, %16, "[1,0,3,2]") ME_FRAC_BFLY(%15, %16, "[1,0,3,2]")
        ME_FRAC_BFLY(%0, %17, "[2,3,0,1]") ME_FRAC_BFLY(%1, %17, "[2,3,0,1]") ME_FRAC_BFLY(%2, %17, "[2,3,0,1]") ME_FRAC_BFLY(%3, %17, "[2,3,0,1]")
        ME_FRAC_BFLY(%4, %17, "[2,3,0,1]") ME_FRAC_BFLY(%5, %17, "[2,3,0,1]") ME_FRAC_BFLY(%6, %17, "[2,3,0,1]") ME_FRAC_BFLY(%7, %17, "[2,3,0,1]")
        ME_FRAC_BFLY(%8, %17, "[2,3,0,1]") ME_FRAC_BFLY(%9, %17, "[2,3,0,1]") ME_FRAC_BFLY(%10, %17, "[2,3,0,1]") ME_FRAC_BFLY(%11, %17, "[2,3,0,1]")
        ME_FRAC_BFLY(%12, %17, "[2,3,0,1]") ME_FRAC_BFLY(%13, %17, "[2,3,0,1]") ME_FRAC_BFLY(%14, %17, "[2,3,0,1]") ME_FRAC_BFLY(%15, %17, "[2,3,0,1]")
        : "+v"(z[0]), "+v"(z[1]), "+v"(z[2]), "+v"(z[3]), "+v"(z[4]), "+v"(z[5]), "+v"(z[6]), "+v"(z[7]), "+v"(z[8]), "+v"(z[9]),
          "+v"(z[10]), "+v"(z[11]), "+v"(z[12]), "+v"(z[13]), "+v"(z[14]), "+v"(z[15])
        : "v"(s1), "v"(s2));
#pragma unroll
    for (int i = 0; i < 8; ++i) { const float t = me_absmax(z[2 * i], z[2 * i + 1]); sum = i ? sum + t : t; }
    sum += sum;
    sum += me_dpp_f(sum, 1);
    sum += me_dpp_f(sum, 0);
    return ((uint32_t)sum + 2) >> 2;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) { const float t = me_absmax(z[2 * i], z[2 * i + 1]); sum = i ? sum + t : t; }
  return (uint32_t)sum;   // (2 * sum + 1) >> 1
}

// The evaluation of one work item.  Stage 0 (me_frac_eval0): the nine half-pel points around the integer MV; stage 1 (me_frac_eval1):
// the eight quarter-pel points around the slot's half-pel winner.  P: patch rows of 3 * BPS dwords, 8-bit samples XORed with 0x80
// (signed bytes p - 128: the 128 * 64 this removes IS the -8192 offset of the first pass).  orgM: current samples + kRoundMagic.
// KIND8: the lane is one quadrant (role 0..3 = TL, TR, BL, BR) of an 8x8 Hadamard block; all four lanes of the quad return the
// block's distortion.  out[point]: distortion of the refinement points in HM's point order (s_acMvRefineH / Q, TEncSearch.cpp:51-75).
// Arithmetic: first pass in integer dot products (v_dot4_i32_i8 / v_dot2c_i32_i16, shift bd-8), second pass, rounding, clipping
// and the Hadamard transform in fp32 -- every value is an integer (or an integer + a fraction of a few bits) below 2^23, so fp32 is
// exact, the order of summation is free, and v_fmac_f32 issues at the full VALU rate where v_mad_i32_i24 does not
// (tools/ubench/valu_rates3).  bd = bit depth of the video (8 when BPS == 1): the two passes shift by bd-8 and 20-bd around the
// 14-bit intermediate (TComInterpolationFilter.cpp:170-212: headRoom = 14 - bd).  Second pass: floor((S + 2^(sh2-1) + (8192 << 6))
// >> sh2) = nearest integer of (S + 524288 + 0.5) * 2^-sh2 (never a tie).  clip_lo: 0, or the bias 2^bd that block and window of a
// bi-prediction origin carry (hmme.hip ctu_call): the taps sum to 64, so a bias B = 2^bd passes both filter stages exactly
// (64 * B >> (bd - 8) = 2^14, 64 * 2^14 >> (20 - bd) = B): the predicted sample comes out as pred + B, is clipped to [B, B + maxv]
// and meets a current sample that carries the same B.
// explicit weighted prediction in the refinement (xGetHADsw / xGetSADw, TComRdCostWeightPrediction.cpp:407-470, :55-90): the interpolated,
// clipped prediction p is weighted sample by sample, pred = ((w0 * p + round) >> shift) + offset, before the difference is taken.
// ws = w0 * 2^-shift, rs = round * 2^-shift: fma(ws, p, rs) IS (w0 * p + round) / 2^shift exactly (|w0 * p + round| < 2^24), v_floor_f32
// the shift; org_sub = what to take off a staged current sample: its staging bias + offset.  WP = 0: none of this is compiled in.
struct FracWp { float ws, rs, org_sub; };
// The item's sixteen current samples (+ kRoundMagic) as the evaluation reads them, row by row: sixteen registers.  (Round 6 put them into a
// block of LDS for the u16 variants, which sit at the 256-VGPR limit and spill 5..9 dwords: nothing spilled any more and 8-10 % slower --
// 24-40 B of scratch per lane cost less than 36 more LDS reads per item.  profiles/r06h_frac_tree_ab.txt)
struct FracOrgRegs {
  const float (&m)[16];
  __device__ __forceinline__ float4 row(int r) const { return make_float4(m[4 * r], m[4 * r + 1], m[4 * r + 2], m[4 * r + 3]); }
};
// a whole-picture launch derives each job itself (me_picture_job: what me_prep_jobs_kernel writes into a job table) -- one kernel
// launch less per refinement; the per-CTU call hands over the job the host prepared
struct FracPrep { const int16_t* pred_q; uint32_t ctus, dims; int sr; };   // ctus: ctu_first | ctu_count << 16; dims: width | height << 16 (few scalar registers: they stay live across the kernel)
constexpr float kRoundMagic = 12582912.0f;   // 1.5 * 2^23: x + magic rounds x to the nearest integer (ties to even)
// First pass on 8-bit planes without v_cvt_f32_i32: the dot-product chain of a filtered sample starts from the BIT PATTERN of
// kRoundMagic (0x4B400000; ulp 1, so adding an integer k, |k| < 2^22, to the pattern gives the pattern of kRoundMagic + k -- here
// |k| <= 128 * 112) and one v_sub_f32 takes the magic off again: v_dot4_i32_i8 (the three-operand form, addend = the magic) +
// v_sub_f32 in place of v_mov_b32 0 + v_dot4c + v_cvt_f32_i32 (13.6 -> 7.7 issue cycles per sample, profiles/r01d_ubench_valu_rates3.txt).
// (clamp = 1 keeps the instruction in its three-operand form -- the accumulating v_dot4c has no clamp bit -- and never clamps here)
__device__ __forceinline__ int me_dot4_magic(uint32_t p, uint32_t t) { return __builtin_amdgcn_sdot4((int)p, (int)t, 0x4B400000, true); }
// STAGE 1 as the kernel runs it: the eight quarter-pel points around the half-pel winner (h3x - 1, h3y - 1) from the 11 x 11 patch that
// starts at the shared window's first sample (me_tap8): HM's two filter passes sample for sample -- the taps left out are zeros.
// P: 11 rows x 11 samples; tab_h / tab_v: [h3 * 3 + offset] rows of 8 taps.
template <int HAD, int BPS, int KIND8, int WP, class Org>
__device__ __forceinline__ void me_frac_eval1(const uint32_t (&P)[kFracRows1][3 * BPS], const Org orgM, int h3x, int h3y, int role, int bd,
                                              float clip_lo, const uint32_t* tab_h, const float* tab_v, bool want4, const FracWp wp,
                                              uint32_t (&out)[9], uint32_t (&out4)[9]) {
  constexpr int PW = 3 * BPS;
  constexpr int idxQ[3][3] = {{3, 1, 4}, {5, 0, 6}, {7, 2, 8}};   // [dy+1][dx+1], s_acMvRefineQ order (reference TEncSearch.cpp:64-75)
  const float s1 = (role & 1) ? -1.f : 1.f, s2 = (role & 2) ? -1.f : 1.f;
  const int sh1 = BPS == 1 ? 0 : bd - 8;
  const int off1 = BPS == 1 ? 0 : -(8192 << sh1);
  const float sc2 = BPS == 1 ? 1.f / 4096.f : __int_as_float((127 - (20 - bd)) << 23);
  const float maxv = clip_lo + (BPS == 1 ? 255.f : (float)((1 << bd) - 1));
  out[0] = 0; out4[0] = 0;   // the centre IS the half-pel winner: carried over by the slot's winner thread, not evaluated again
#pragma unroll
  for (int dxi = 0; dxi < 3; ++dxi) {
    const uint32_t* row = tab_h + (h3x * 3 + dxi) * kFracTabH;
    float tmp[kFracRows1][4];   // first pass into the 14-bit intermediates
    if constexpr (BPS == 1) {
      // output column c reads bytes c .. c + 7 of the row: the packed taps moved up by c bytes (column 0 stays inside two dwords)
      const uint32_t w0 = row[0], w1 = row[1];
      uint32_t T[4][3];
      T[0][0] = w0; T[0][1] = w1; T[0][2] = 0;
#pragma unroll
      for (int c = 1; c < 4; ++c) {
        T[c][0] = w0 << (8 * c);
        T[c][1] = __builtin_amdgcn_alignbyte(w1, w0, 4 - c);
        T[c][2] = w1 >> (8 * (4 - c));
      }
#pragma unroll
      for (int r = 0; r < kFracRows1; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          int a = me_dot4_magic(P[r][0], T[c][0]);
          a = __builtin_amdgcn_sdot4((int)P[r][1], (int)T[c][1], a, false);
          if (c > 0) a = __builtin_amdgcn_sdot4((int)P[r][2], (int)T[c][2], a, false);
          tmp[r][c] = __int_as_float(a) - kRoundMagic;
        }
    } else {
      typedef short v2s __attribute__((ext_vector_type(2)));
      uint32_t w[4], h[5];   // h: the taps moved up by one sample
#pragma unroll
      for (int k = 0; k < 4; ++k) w[k] = row[k];
      h[0] = w[0] << 16;
#pragma unroll
      for (int k = 1; k < 4; ++k) h[k] = __builtin_amdgcn_alignbyte(w[k], w[k - 1], 2);
      h[4] = w[3] >> 16;
#pragma unroll
      for (int r = 0; r < kFracRows1; ++r) {
        int a0 = off1, a1 = off1, a2 = off1, a3 = off1;   // columns 0..3: samples c .. c + 7 = dwords c / 2 .. (c + 7) / 2
#pragma unroll
        for (int k = 0; k < 4; ++k) a0 = __builtin_amdgcn_sdot2(__builtin_bit_cast(v2s, P[r][k]), __builtin_bit_cast(v2s, w[k]), a0, false);
#pragma unroll
        for (int k = 0; k < 5; ++k) a1 = __builtin_amdgcn_sdot2(__builtin_bit_cast(v2s, P[r][k]), __builtin_bit_cast(v2s, h[k]), a1, false);
#pragma unroll
        for (int k = 0; k < 4; ++k) a2 = __builtin_amdgcn_sdot2(__builtin_bit_cast(v2s, P[r][k + 1]), __builtin_bit_cast(v2s, w[k]), a2, false);
#pragma unroll
        for (int k = 0; k < 5; ++k) a3 = __builtin_amdgcn_sdot2(__builtin_bit_cast(v2s, P[r][k + 1]), __builtin_bit_cast(v2s, h[k]), a3, false);
        tmp[r][0] = (float)(a0 >> sh1); tmp[r][1] = (float)(a1 >> sh1); tmp[r][2] = (float)(a2 >> sh1); tmp[r][3] = (float)(a3 >> sh1);
      }
    }
#pragma unroll
    for (int dyi = 0; dyi < 3; ++dyi) {
      if (dxi == 1 && dyi == 1) continue;
      float cv[8];   // taps * 2^-sh2 (exact): the accumulator is the sample value with its fraction
#pragma unroll
      for (int j = 0; j < 8; ++j) cv[j] = tab_v[(h3y * 3 + dyi) * kFracTabV + j];
      float d[16];
      v2f dp[4][2];
      if constexpr (!WP) {   // two columns per instruction: v_pk_fma_f32 / v_pk_add_f32
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float4 org = orgM.row(r);
#pragma unroll
          for (int cp = 0; cp < 2; ++cp) {
            v2f a = {524288.5f * sc2, 524288.5f * sc2};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const v2f t = {tmp[r + j][2 * cp], tmp[r + j][2 * cp + 1]}, cc = {cv[j], cv[j]};
              a = __builtin_elementwise_fma(cc, t, a);
            }
            const v2f y = v2f{__builtin_amdgcn_fmed3f(a.x, clip_lo, maxv), __builtin_amdgcn_fmed3f(a.y, clip_lo, maxv)} + v2f{kRoundMagic, kRoundMagic};
            const v2f dd = (cp ? v2f{org.z, org.w} : v2f{org.x, org.y}) - y;
            d[4 * r + 2 * cp] = dd.x; d[4 * r + 2 * cp + 1] = dd.y;
            dp[r][cp] = dd;
          }
        }
      } else
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float4 org = orgM.row(r);
        const float og[4] = {org.x, org.y, org.z, org.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          float a = 524288.5f * sc2;   // second pass (TComInterpolationFilter.cpp:195-212)
#pragma unroll
          for (int j = 0; j < 8; ++j) a = __builtin_fmaf(cv[j], tmp[r + j][c], a);
          const float y = __builtin_amdgcn_fmed3f(a, clip_lo, maxv) + kRoundMagic;   // clip, then round (the bounds are integers)
          d[4 * r + c] = og[c] - (WP ? __builtin_floorf(__builtin_fmaf(wp.ws, y - kRoundMagic, wp.rs)) : y);
        }
      }
      uint32_t own4 = 0;
      const uint32_t contrib = (HAD && !WP) ? me_frac_had_pk<KIND8>(dp, s1, s2, want4, own4) : me_frac_dist<HAD, KIND8>(d, s1, s2, want4, own4);
      out[idxQ[dyi][dxi]] = contrib;
      out4[idxQ[dyi][dxi]] = own4;
    }
  }
}

// Work sharing.  A kind-8 slot (width and height multiples of 8) is a set of 8x8 Hadamard blocks, any other slot a set
// of 4x4 blocks; each of the 64 8x8 positions of the CTU is covered by kFracCover8 = 18 kind-8 slots (7 partition modes
// at 64 and 32, three at 16, one at 8) and each of the 256 4x4 positions by kFracCover4 = 6 others (the 4 AMP shapes at
// 16, 8x4, 4x8).  Slots that cover a position with the same integer MV (and, in the quarter-pel stage, the same half-pel
// winner) get the same nine distortions from it, so each stage first lists the DISTINCT (position, MV) pairs, evaluates
// those -- one lane per 4x4 block, a quad of lanes per 8x8 block -- and adds the result to every slot that shares it.
// `cover`: uint16 [64][18] then [256][6] slot ids, ascending (built by the host from the slot table).
constexpr int kFracCover8 = 18, kFracCover4 = 6, kFracPairs8 = 64 * kFracCover8, kFracPairs4 = 256 * kFracCover4;
// slot state word: (mx - lt_x) | (my - lt_y) << 9 | (half_x + 1) << 18 | (half_y + 1) << 20; the sharing key of a stage
constexpr uint32_t kFracKey0 = 0x3ffffu, kFracKey1 = 0x3fffffu;

// `src`: window sample (-4,-4) of this CTU in the reference plane, `gpitch` bytes per row.  The 12x12 patch (11x11 in the quarter-pel stage) comes straight
// from global memory: the windows of neighbouring CTUs overlap and stay in L2, and an LDS copy of the window (tried first)
// was no faster while it capped the search range at 64 and the occupancy at one 16-bit workgroup per CU.
// STAGE 0 (the nine half-pel points) with the filters SHARED between the points that use them.  The half-pel sample to the right of
// integer column x is the half-pel sample to the left of x + 1, and likewise for rows: the horizontal half-pel pass is computed for five
// columns (HH[r][k], k = 0..4: the samples left of columns 0..3 and right of column 3) instead of 2 x 4, the vertical half-pel pass for
// five rows of each column (rows above 0..3 and below 3) instead of 2 x 4, and every filtered value is rounded and clipped once, not once
// per point that reads it: 396 second-pass FMAs instead of 816, 165 first-pass dot products instead of 264.  Same values as nine
// separate evaluations bit for bit: every intermediate is exact in fp32 (above), so the order of summation is free.
template <int HAD, int BPS, int KIND8, int WP, class Org>
__device__ __forceinline__ void me_frac_eval0(const uint32_t (&P)[12][3 * BPS], const Org orgM, int role, int bd, float clip_lo,
                                              bool want4, const FracWp wp, uint32_t (&out)[9], uint32_t (&out4)[9]) {
  constexpr int PW = 3 * BPS;
  constexpr int idxH[3][3] = {{5, 1, 6}, {3, 0, 4}, {7, 2, 8}};   // [dy+1][dx+1], s_acMvRefineH order (TEncSearch.cpp:51-75)
  const float s1 = (role & 1) ? -1.f : 1.f, s2 = (role & 2) ? -1.f : 1.f;
  const int sh1 = BPS == 1 ? 0 : bd - 8;
  const int off1 = BPS == 1 ? 0 : -(8192 << sh1);
  const float sc2 = BPS == 1 ? 1.f / 4096.f : __int_as_float((127 - (20 - bd)) << 23);
  const float maxv = clip_lo + (BPS == 1 ? 255.f : (float)((1 << bd) - 1));
  const float init = 524288.5f * sc2;
  float cv[8];                                  // half-pel taps * 2^-sh2
#pragma unroll
  for (int t = 0; t < 8; ++t) cv[t] = (float)me_luma_tap(2, t) * sc2;
  const float c64 = 64.f * sc2;
  // first pass of patch row r with the tap window of (quarter offset q, output column c)
  auto first = [&](int r, int q, int c) -> float {
    if constexpr (BPS == 1) {
      int a = 0;
      bool started = false;
#pragma unroll
      for (int k = 0; k < PW; ++k) {
        if (me_htap_dw<BPS>(q, c, k) == 0) continue;
        a = started ? __builtin_amdgcn_sdot4((int)P[r][k], (int)me_htap_dw<BPS>(q, c, k), a, false) : me_dot4_magic(P[r][k], me_htap_dw<BPS>(q, c, k));
        started = true;
      }
      return __int_as_float(a) - kRoundMagic;
    } else {
      typedef short v2s __attribute__((ext_vector_type(2)));
      int a = off1;
#pragma unroll
      for (int k = 0; k < PW; ++k) {
        if (me_htap_dw<BPS>(q, c, k) == 0) continue;
        a = __builtin_amdgcn_sdot2(__builtin_bit_cast(v2s, P[r][k]), __builtin_bit_cast(v2s, me_htap_dw<BPS>(q, c, k)), a, false);
      }
      return (float)(a >> sh1);
    }
  };
  auto clipround = [&](float a) -> float {
    const float y = __builtin_amdgcn_fmed3f(a, clip_lo, maxv) + kRoundMagic;
    return WP ? __builtin_floorf(__builtin_fmaf(wp.ws, y - kRoundMagic, wp.rs)) : y;   // WP: orgM carries no magic either (me_frac_compute)
  };
  // one point: d = org - pred over the 4x4 block, pred(r, c) = y[r0 + r][c0 + c]
#define ME_FRAC_POINT(Y, R0, C0, DYI, DXI)                                                   \
  {                                                                                          \
    float d[16];                                                                             \
    _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                          \
      const float4 org_ = orgM.row(r);                                                       \
      const float og_[4] = {org_.x, org_.y, org_.z, org_.w};                                 \
      _Pragma("unroll") for (int c = 0; c < 4; ++c) d[4 * r + c] = og_[c] - Y[(R0) + r][(C0) + c]; \
    }                                                                                        \
    uint32_t own4 = 0;                                                                       \
    out[idxH[DYI][DXI]] = me_frac_dist<HAD, KIND8>(d, s1, s2, want4, own4);                  \
    out4[idxH[DYI][DXI]] = own4;                                                             \
  }
  // ---- half-pel columns: HH[r][k] = horizontal half-pel sample left of column k (k = 0..3) / right of column 3 (k = 4)
  {
    float HH[12][5];
#pragma unroll
    for (int r = 0; r < 12; ++r) {
#pragma unroll
      for (int k = 0; k < 4; ++k) HH[r][k] = first(r, -2, k);
      HH[r][4] = first(r, 2, 3);
    }
    float yG[5][5], yZ[4][5];                     // vertical half-pel rows above 0..3 and below 3 / the integer rows
#pragma unroll
    for (int k = 0; k < 5; ++k) {
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        float a = init;
#pragma unroll
        for (int t = 0; t < 8; ++t) a = __builtin_fmaf(cv[t], HH[j + t][k], a);
        yG[j][k] = clipround(a);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) yZ[r][k] = clipround(__builtin_fmaf(c64, HH[r + 4][k], init));
    }
    ME_FRAC_POINT(yG, 0, 0, 0, 0) ME_FRAC_POINT(yG, 0, 1, 0, 2) ME_FRAC_POINT(yG, 1, 0, 2, 0) ME_FRAC_POINT(yG, 1, 1, 2, 2)
    ME_FRAC_POINT(yZ, 0, 0, 1, 0) ME_FRAC_POINT(yZ, 0, 1, 1, 2)
  }
  // ---- integer columns
  if constexpr (!WP) {
    // the first pass of an integer column is (64 * p - (8192 << sh1)) >> sh1 = p * 2^(6 - sh1) - 8192: the sample itself goes into the
    // vertical filter (v_cvt_f32_ubyteN of the raw byte / a conversion of the 16-bit half), the taps carry the 2^(6 - sh1) and the
    // constant the -8192 -- the same real number, exact in fp32 like the general form.  The integer-position sample needs neither
    // filter nor clip: it is a sample of the window (with the window's bias, if any), inside [clip_lo, maxv] as it stands.  Weighted
    // calls take the general form below: their integer-position prediction is weighted like the others
    float V0[12][4];
#pragma unroll
    for (int r = 0; r < 12; ++r) {
      if constexpr (BPS == 1) {
        const uint32_t raw = P[r][1] ^ 0x80808080u;   // patch columns 4..7 = block columns 0..3
#pragma unroll
        for (int c = 0; c < 4; ++c) V0[r][c] = (float)((raw >> (8 * c)) & 0xff);
      } else {
        V0[r][0] = (float)(P[r][2] & 0xffff); V0[r][1] = (float)(P[r][2] >> 16);
        V0[r][2] = (float)(P[r][3] & 0xffff); V0[r][3] = (float)(P[r][3] >> 16);
      }
    }
    const float up = (float)(64 >> sh1);
    float cw[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) cw[t] = cv[t] * up;
    const float init_i = init - 8192.f * 64.f * sc2;
    float yG[5][4], yZ[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        float a = init_i;
#pragma unroll
        for (int t = 0; t < 8; ++t) a = __builtin_fmaf(cw[t], V0[j + t][c], a);
        yG[j][c] = clipround(a);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) yZ[r][c] = V0[r + 4][c] + kRoundMagic;
    }
    ME_FRAC_POINT(yG, 0, 0, 0, 1) ME_FRAC_POINT(yG, 1, 0, 2, 1) ME_FRAC_POINT(yZ, 0, 0, 1, 1)
  } else {
    float V0[12][4];
#pragma unroll
    for (int r = 0; r < 12; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) V0[r][c] = first(r, 0, c);
    float yG[5][4], yZ[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        float a = init;
#pragma unroll
        for (int t = 0; t < 8; ++t) a = __builtin_fmaf(cv[t], V0[j + t][c], a);
        yG[j][c] = clipround(a);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) yZ[r][c] = clipround(__builtin_fmaf(c64, V0[r + 4][c], init));
    }
    ME_FRAC_POINT(yG, 0, 0, 0, 1) ME_FRAC_POINT(yG, 1, 0, 2, 1) ME_FRAC_POINT(yZ, 0, 0, 1, 1)
  }
#undef ME_FRAC_POINT
}

// One work item = one 4x4 block of one (position, MV) pair; `pair` indexes the cover table (kind-8 pairs first), `role` is the lane's
// quadrant of an 8x8 Hadamard block.  An item is handled in two steps:
//   me_frac_fetch    slot state + address -> 12 raw rows of PW + 1 aligned dwords each (global_load_dwordx4 / x3), nothing waited for
//   me_frac_compute  byte-align the rows (first use = the wait), evaluate the 9 / 8 points, add to the slots that share the key
template <int BPS>
struct FracRaw {
  uint32_t w[12][3 * BPS + 1];
  uint32_t sv;      // state word of the item's first slot (the sharing key of the stage)
  uint32_t o;       // byte offset of the patch inside its first dword
};

template <int STAGE, int BPS, int KIND8>
__device__ __forceinline__ void me_frac_fetch(const uint8_t* __restrict__ src, int gpitch, const uint32_t* st, const uint16_t* cover, int pair, int role,
                                              FracRaw<BPS>& R) {
  constexpr int PW = 3 * BPS, NCOV = KIND8 ? kFracCover8 : kFracCover4;
  const int q = KIND8 ? pair : pair - kFracPairs8;
  const int pos = q / NCOV;
  const uint32_t sv = st[cover[pair]];
  const int bx = KIND8 ? 2 * (pos & 7) + (role & 1) : (pos & 15), by = KIND8 ? 2 * (pos >> 3) + (role >> 1) : (pos >> 4);
  // patch (0,0) = block sample (-4,-4) = window row (by*4 + my - lt_y), sample (bx*4 + mx - lt_x) (halo offsets cancel); in the
  // quarter-pel stage the patch starts at the first sample of the component's shared 8-tap window (me_win8_first): (-4 or -3, -4 or -3)
  const int skip_x = STAGE ? 4 + me_win8_first((int)((sv >> 18) & 3)) : 0, skip_y = STAGE ? 4 + me_win8_first((int)((sv >> 20) & 3)) : 0;
  const int prow = by * 4 + (int)((sv >> 9) & 0x1ff) + skip_y, pcol = (bx * 4 + (int)(sv & 0x1ff) + skip_x) * BPS;   // pcol in bytes
  const uint8_t* a = src + (long)prow * gpitch + pcol;
  const uint32_t o = (uint32_t)(uintptr_t)a & 3u;
  const uint32_t* __restrict__ rowp = (const uint32_t*)(a - o);
  const int gp = gpitch >> 2;
  // 11 u16 samples and their alignment fill six dwords at most; the seventh only feeds sample 11, which no tap reads
  constexpr int ROWS = STAGE ? kFracRows1 : 12, NL = (STAGE && BPS == 2) ? PW : PW + 1;
#pragma unroll
  for (int r = 0; r < ROWS; ++r)
#pragma unroll
    for (int k = 0; k <= PW; ++k) R.w[r][k] = k < NL ? rowp[r * gp + k] : 0u;
  R.sv = sv;
  R.o = o;
}

template <int STAGE, int HAD, int BPS, int KIND8, int WP>
__device__ __forceinline__ void me_frac_compute(const FracRaw<BPS>& R, const uint32_t* curl, const uint32_t* st, const uint16_t* cover, int pair, int role,
                                                int bd, float clip_lo, const FracWp wp, const uint32_t* tab_h, const float* tab_v, uint32_t* acc, bool ride) {
  constexpr int PW = 3 * BPS, NCOV = KIND8 ? kFracCover8 : kFracCover4;
  constexpr uint32_t keymask = STAGE ? kFracKey1 : kFracKey0;
  const int q = KIND8 ? pair : pair - kFracPairs8;
  const int pos = q / NCOV, j = q - pos * NCOV;
  const uint16_t* cov = cover + (KIND8 ? 0 : kFracPairs8) + pos * NCOV;
  const uint32_t sv = R.sv;
  const int bx = KIND8 ? 2 * (pos & 7) + (role & 1) : (pos & 15), by = KIND8 ? 2 * (pos >> 3) + (role >> 1) : (pos >> 4);
  constexpr int ROWS = STAGE ? kFracRows1 : 12;
  uint32_t P[ROWS][PW];
#pragma unroll
  for (int r = 0; r < ROWS; ++r)
#pragma unroll
    for (int k = 0; k < PW; ++k) P[r][k] = __builtin_amdgcn_alignbyte(R.w[r][k + 1], R.w[r][k], R.o) ^ (BPS == 1 ? 0x80808080u : 0u);
  float orgM[16];   // current samples + kRoundMagic (exact: integers below 2^24); WP: current samples - staging bias - offset, no magic
  const float org_add = WP ? -wp.org_sub : kRoundMagic;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if constexpr (BPS == 1) {
      const uint32_t w = curl[(by * 4 + r) * 16 + bx];
#pragma unroll
      for (int c = 0; c < 4; ++c) orgM[4 * r + c] = (float)((w >> (8 * c)) & 0xff) + org_add;
    } else {
      const uint2 w = *(const uint2*)&curl[(by * 4 + r) * 32 + bx * 2];
      orgM[4 * r] = (float)(w.x & 0xffff) + org_add; orgM[4 * r + 1] = (float)(w.x >> 16) + org_add;
      orgM[4 * r + 2] = (float)(w.y & 0xffff) + org_add; orgM[4 * r + 3] = (float)(w.y >> 16) + org_add;
    }
  }
  uint32_t dist[9], dist4[9];
  // Slots made of 4x4 blocks (the AMP shapes at 16, 8x4, 4x8: six per 4x4 position) whose key equals this item's get this lane's 4x4
  // block for nothing: same patch, same interpolated samples, same difference, same 4x4 transform -- the work-list pass left such
  // (4x4 position, key) pairs out of the 4x4 list (me_frac_dedupe4).  On coherent content that is every one of them.
  // `ride` (wave-uniform): only a position's IMPLICIT item carries riders.  A listed kind-8 item used to as well; but one rider in a
  // wave makes all 64 lanes compute their own 4x4 sums at all nine points (7 % of an item), and on content whose slots do not share
  // their motion nearly every wave had one and nearly no lane needed it -- as an item of its own that rider costs one LANE of a wave.
  uint32_t match4 = 0;
  const uint16_t* cov4 = cover + kFracPairs8 + (by * 16 + bx) * kFracCover4;
  if (KIND8 && ride) {
#pragma unroll
    for (int k = 0; k < kFracCover4; ++k) match4 |= (((st[cov4[k]] ^ sv) & keymask) == 0 ? 1u : 0u) << k;
  }
  const bool want4 = KIND8 && __any(match4 != 0);
  {
    const FracOrgRegs org = {orgM};
    if constexpr (STAGE == 0) me_frac_eval0<HAD, BPS, KIND8, WP>(P, org, role, bd, clip_lo, want4, wp, dist, dist4);
    else me_frac_eval1<HAD, BPS, KIND8, WP>(P, org, (int)((sv >> 18) & 3), (int)((sv >> 20) & 3), role, bd, clip_lo, tab_h, tab_v, want4, wp, dist, dist4);
  }
  // the nine (stage 1: eight, point 0 is carried over, not evaluated -- its distortion here is 0) distortions as they are added to a slot
  unsigned long long pk[3], pk4[3];
  if constexpr (frac_pack3(BPS)) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      pk[k] = (unsigned long long)(dist[3 * k] | dist[3 * k + 1] << 21) | (unsigned long long)(dist[3 * k + 1] >> 11 | dist[3 * k + 2] << 10) << 32;
      pk4[k] = (unsigned long long)(dist4[3 * k] | dist4[3 * k + 1] << 21) | (unsigned long long)(dist4[3 * k + 1] >> 11 | dist4[3 * k + 2] << 10) << 32;
    }
  }
  auto add_to = [&](int slot, const uint32_t (&d)[9], const unsigned long long (&p)[3]) {
    if constexpr (frac_pack3(BPS)) {
      unsigned long long* a = (unsigned long long*)acc + slot * 3;
#pragma unroll
      for (int k = 0; k < 3; ++k) atomicAdd(&a[k], p[k]);
    } else {
#pragma unroll
      for (int i = STAGE; i < 9; ++i) atomicAdd(&acc[slot * 9 + i], d[i]);
    }
  };
  if (KIND8 && want4) {
#pragma unroll
    for (int k = 0; k < kFracCover4; ++k)
      if (match4 >> k & 1) add_to(cov4[k], dist4, pk4);
  }
  // Every slot of this position with the same key takes the distortions; the quad's lanes split the slot list.
  // (Round 3 tried to relieve these adds -- the large slots cover many positions, so lanes of one wave often add to the same address:
  // each quad starting its walk at another list position and two points per ds_add_u64 cut the kernel's LDS conflict cycles by 27 %
  // and its LDS waits by 90 %, and changed its time by -2 % .. +3 %: LDS is busy 10 % of the CU cycles here.  profiles/archive/r03d_frac_ab.txt)
  // (slot ids first, then their keys, then the adds: two LDS round trips for the lane's whole share -- walking the list entry by entry
  // was two dependent round trips PER entry at the end of every item, with nothing else for the wave to issue)
  {
    constexpr int STEP = KIND8 ? 4 : 1, MAXN = KIND8 ? 5 : kFracCover4;
    const int j0 = j + (KIND8 ? role : 0);
    int s2[MAXN];
    uint32_t k2[MAXN];
#pragma unroll
    for (int k = 0; k < MAXN; ++k) s2[k] = cov[min(j0 + k * STEP, NCOV - 1)];
#pragma unroll
    for (int k = 0; k < MAXN; ++k) k2[k] = st[s2[k]];
#pragma unroll
    for (int k = 0; k < MAXN; ++k) {
      const int j2 = j0 + k * STEP;
      if (j2 < NCOV && (j2 == j || ((k2[k] ^ sv) & keymask) == 0)) add_to(s2[k], dist, pk);
    }
  }
}

// distinct (position, key) pairs of one stage -> work lists; the first slot (lowest index in the cover list) with a given key is the one
// evaluated.  Entry 0 of a position's list -- its 8x8 slot -- is always a first: it is the position's IMPLICIT item (me_frac_stage) and never
// listed.  PARTS waves share a position's list: part PART decides entries PART, PART + PARTS, ... (an 8x8 position's 18 entries are
// 153 compares: one wave per part -- the part is wave-uniform, so each wave runs only its own 32..45 compares -- keeps the four
// waves of the workgroup equally busy).  A wave whose 64 positions each have ONE key (slots that share their motion: most of a real
// picture) has nothing to list and skips the compares.
template <int NCOV, int PARTS, int PART>
__device__ __forceinline__ void me_frac_dedupe(const uint32_t* st, const uint16_t* cov, uint32_t keymask, int pair0,
                                               uint32_t* counter, uint16_t* list) {
  uint32_t key[NCOV];
#pragma unroll
  for (int j = 0; j < NCOV; ++j) key[j] = st[cov[j]] & keymask;
  uint32_t differ = 0;
#pragma unroll
  for (int j = 1; j < NCOV; ++j) differ |= key[j] ^ key[0];
  if (__all(differ == 0)) return;
#pragma unroll
  for (int j = PART ? PART : PARTS; j < NCOV; j += PARTS) {
    bool first = true;
#pragma unroll
    for (int k = 0; k < j; ++k) first = first && key[k] != key[j];
    if (first) list[atomicAdd(counter, 1u)] = (uint16_t)(pair0 + j);
  }
}

// the 4x4 kind: a (4x4 position, key) pair is listed unless its key is that of the position's 8x8 slot -- then the lane of the position's
// implicit item that owns this 4x4 block hands its result to the 4x4-kind slots as well (me_frac_compute, `ride`)
__device__ __forceinline__ void me_frac_dedupe4(const uint32_t* st, const uint16_t* cover, int p4, uint32_t keymask, uint32_t* counter, uint16_t* list) {
  const uint16_t* cov = cover + kFracPairs8 + p4 * kFracCover4;
  const uint16_t* cov8 = cover + (((p4 >> 4) >> 1) * 8 + ((p4 & 15) >> 1)) * kFracCover8;   // the 8x8 position that holds block (p4 & 15, p4 >> 4)
  uint32_t key[kFracCover4];
  bool first[kFracCover4];
  const uint32_t k80 = st[cov8[0]] & keymask;
  uint32_t differ = 0;
#pragma unroll
  for (int j = 0; j < kFracCover4; ++j) {
    key[j] = st[cov[j]] & keymask;
    differ |= key[j] ^ k80;
  }
  if (__all(differ == 0)) return;   // every 4x4-kind slot of the wave's positions rides on its position's implicit 8x8 item
#pragma unroll
  for (int j = 0; j < kFracCover4; ++j) {
    first[j] = key[j] != k80;
#pragma unroll
    for (int k = 0; k < j; ++k) first[j] = first[j] && key[k] != key[j];
  }
#pragma unroll
  for (int j = 0; j < kFracCover4; ++j)
    if (first[j]) list[atomicAdd(counter, 1u)] = (uint16_t)(kFracPairs8 + p4 * kFracCover4 + j);
}

// One stage's items.  Every 8x8 position has an item that needs no list: entry 0 of its cover list (the 8x8 slot itself) with that slot's
// key -- 64 positions x 4 quadrants = one item for each of the 256 lanes.  A lane requests that item's patch rows FIRST, builds its share
// of the work lists (the remaining distinct (position, key) pairs) while the rows are on their way, evaluates the item, and only then meets
// the other waves at the barrier that completes the lists.  On content whose slots share their motion the lists stay empty and a stage is
// one item per lane; the list phase used to be a barrier-separated 2.5 .. 3.5 us of dependent LDS round trips in front of every stage's
// items (profiles/r05k_frac_phases_before_after.txt).  The listed items follow: kind-8 items (whole quads), then kind-4 items.  (Round 4 built the walk
// over the listed items software-pipelined -- the next item's rows requested before the current item is evaluated -- slower on every content,
// profiles/r04a_frac_pipelined_vs_plain_ab.txt.)
template <int STAGE, int HAD, int BPS, int WP>
__device__ __forceinline__ void me_frac_stage(const uint8_t* __restrict__ src, int gpitch, const uint32_t* curl, const uint32_t* st, const uint16_t* cover,
                                              uint16_t* list8, uint16_t* list4, uint32_t* counter, uint32_t* pf, int tid, int bd, float clip_lo,
                                              const FracWp wp, const uint32_t* tab_h, const float* tab_v, uint32_t* acc) {
  constexpr int NT = frac_threads(BPS);
  static_assert(NT == 256, "me_frac_stage: one implicit item per lane (64 positions x 4 quadrants), the work-list pass on 4 waves");
  constexpr uint32_t keymask = STAGE ? kFracKey1 : kFracKey0;
  const int role = tid & 3;
  // the work lists: 64 8x8 positions x 4 waves (wave w decides entries w, w + 4, ... of each position's list), then 256 4x4 positions
  auto lists = [&]() {
    const int p8 = tid & 63;
    const uint16_t* c8 = cover + p8 * kFracCover8;
    switch (__builtin_amdgcn_readfirstlane(tid >> 6)) {
      case 0: me_frac_dedupe<kFracCover8, 4, 0>(st, c8, keymask, p8 * kFracCover8, &counter[0], list8); break;
      case 1: me_frac_dedupe<kFracCover8, 4, 1>(st, c8, keymask, p8 * kFracCover8, &counter[0], list8); break;
      case 2: me_frac_dedupe<kFracCover8, 4, 2>(st, c8, keymask, p8 * kFracCover8, &counter[0], list8); break;
      default: me_frac_dedupe<kFracCover8, 4, 3>(st, c8, keymask, p8 * kFracCover8, &counter[0], list8); break;
    }
    me_frac_dedupe4(st, cover, tid, keymask, &counter[1], list4);
  };
  // (the listed items in chunks of 64 lanes drawn from a counter by the four waves were measured too: no better than this static walk
  // on mixed content, 1 % worse on unrelated pictures, and 14-46 spilled dwords in the u16 kernels)
  int n8 = 0;
#pragma unroll 1
  for (int i8 = tid - NT;; i8 += NT) {   // first turn (i8 < 0 in every lane): the implicit item
    int pair = (tid >> 2) * kFracCover8;
    if (i8 >= 0) {
      if (i8 >= n8) break;
      pair = list8[i8 >> 2];
    }
    FracRaw<BPS> R;
    me_frac_fetch<STAGE, BPS, 1>(src, gpitch, st, cover, pair, role, R);
    if (i8 < 0) {   // the work lists, while the implicit item's rows are on their way
      lists();
      __builtin_amdgcn_s_setprio(0);
    }
    me_frac_compute<STAGE, HAD, BPS, 1, WP>(R, curl, st, cover, pair, role, bd, clip_lo, wp, tab_h, tab_v, acc, i8 < 0);
    if (i8 < 0) {
      __syncthreads();   // the work lists are complete
      n8 = 4 * (int)counter[0];
    }
  }
  const int n4 = (int)counter[1];
  // (dealt from the last thread down: the partly filled last turn of the kind-8 walk above falls on the first waves, this one's on
  // the last -- the waves reach the barrier that ends the stage closer together)
#pragma unroll 1
  for (int i4 = NT - 1 - tid; i4 < n4; i4 += NT) {
    const int pair = list4[i4];
    FracRaw<BPS> R;
    me_frac_fetch<STAGE, BPS, 0>(src, gpitch, st, cover, pair, 0, R);
    me_frac_compute<STAGE, HAD, BPS, 0, WP>(R, curl, st, cover, pair, 0, bd, clip_lo, wp, tab_h, tab_v, acc, false);
  }
  __builtin_amdgcn_s_setprio(3);
}

// Which job the k-th workgroup (or the k-th draw from the job counter) takes.  A launch ends one job time after its last job STARTS, and
// the CTUs on the picture's edge are the slow ones: their slots reach into the padding (a partial bottom row most of all: 2160 = 33 x 64
// + 48), find MVs of their own there and share little -- 2-3 x the time of an interior CTU (profiles/r04k_frac_timeline.txt: the bottom
// row dealt last kept a 2160p launch alive for an extra job time; profiles/r05k_frac_phases_before_after.txt: so did the TOP row once the table
// was simply dealt from its end).  So the edge CTUs of every pair go first -- bottom row, top row, left and right column -- then the
// interiors.  Launches over a CTU sub-range (and pictures less than three CTUs wide or high) keep the plain last-first order.
__host__ __device__ inline int me_frac_deal(int k, int n_jobs, const FracPrep& prep) {
  const int first = (int)(prep.ctus & 0xffff), count = (int)(prep.ctus >> 16);
  const int X = ((int)(prep.dims & 0xffff) + 63) >> 6, Y = ((int)(prep.dims >> 16) + 63) >> 6, n_ctu = X * Y;
  if (first != 0 || count != n_ctu || X < 3 || Y < 3 || n_jobs % n_ctu) return n_jobs - 1 - k;
  const int E = 2 * X + 2 * (Y - 2), I = n_ctu - E, pairs = n_jobs / n_ctu;
  int pair, ctu;
  if (k < pairs * E) {
    pair = k / E;
    int e = k - pair * E;
    if (e < X) ctu = (Y - 1) * X + e;
    else if (e < 2 * X) ctu = e - X;
    else { e -= 2 * X; ctu = (1 + (e >> 1)) * X + ((e & 1) ? X - 1 : 0); }
  } else {
    const int m = k - pairs * E;
    pair = m / I;
    const int i = m - pair * I;
    ctu = (1 + i / (X - 2)) * X + 1 + i % (X - 2);
  }
  return pair * n_ctu + ctu;
}

// WAVES: waves per SIMD the register budget is cut for.  The kernel runs at two (8-bit planes: 237 VGPRs, nothing spilled; two workgroups
// per CU).  Round 4 also ran the 8-bit kernel at three waves for large launches (168 VGPRs + 50 spilled dwords per lane: 104 MB of
// scratch writes per 2160p launch); the round-5 flow made the two-wave build the faster one on content that shares its motion and
// the only one without scratch -- on unrelated pictures the third wave's occupancy would still be worth 6 %.
template <int HAD, int BPS, int WP, int WAVES = 2>
__global__ void __launch_bounds__(frac_threads(BPS), WAVES)
me_frac_kernel(const RefSet curs, int cur_pitch, const RefSet refs, int ref_pitch,
               const MeJob* __restrict__ jobs, const FracPrep prep, int n_jobs, uint32_t* __restrict__ job_counter, const uint16_t* __restrict__ cover_g,
               const int16_t* __restrict__ int_mv, uint32_t lambda_q16, int bit_depth_bias, const FracWp wp, int16_t* __restrict__ out_qmv,
               uint32_t* __restrict__ out_cost) {
  // bit_depth_bias: bit depth in the low 8 bits; bit 8 set = block and window carry the bias 2^bitDepth of a bi-prediction origin
  // (2*org - pred, TEncSearch.cpp:3702-3712: current samples in [-maxv, 2*maxv]; per-CTU calls only, u16 staging)
  const int bit_depth = bit_depth_bias & 0xff;
  static_assert(BPS == 2 || !WP, "weighted calls and bi-prediction origins stage u16 samples (hmme.hip ctu_call)");
  const float clip_lo = (BPS == 2 && (bit_depth_bias & 0x100)) ? (float)(1 << bit_depth) : 0.f;
  constexpr int NT = frac_threads(BPS);
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  uint32_t* acc = smem;                 // [593][frac_acc_row(BPS)] distortion sums of the current stage (8-bit planes: three packed 64-bit words per slot)
  uint32_t* st = smem + frac_acc_dw(BPS);   // [593] slot state: (mx - lt_x) | (my - lt_y) << 9 | (half_x + 1) << 18 | (half_y + 1) << 20
  uint32_t* tab_h = st + 600;           // [9][kFracTabH] packed horizontal taps of the quarter-pel stage: row = (half-pel winner + 1) * 3 + (offset + 1), me_tap8
  float* tab_v = (float*)(tab_h + 9 * kFracTabH);   // [9][kFracTabV] vertical taps, same rows
  uint32_t* counter = tab_h + 152;      // [2] lengths of the two work lists
  uint16_t* list8 = (uint16_t*)(tab_h + 160);                  // distinct (8x8 position, key) pairs
  uint16_t* list4 = (uint16_t*)(tab_h + 160 + kFracPairs8 / 2);   // distinct (4x4 position, key) pairs
  uint32_t* curl = tab_h + 160 + (kFracPairs8 + kFracPairs4) / 2;   // 64 x 64 current block
  uint16_t* cover = (uint16_t*)(curl + 1024 * BPS);   // the cover table (uint16 [64][18] then [256][6]): read per item and per dedupe, so it lives here
  uint32_t* pf = (uint32_t*)(cover + kFracPairs8 + kFracPairs4);   // unused since the patch-row prefetch was removed (dropping it renames IR labels
                                                                   // in build/*.s: left for a change of its own)

  const int tid = threadIdx.x;
  const int bd = BPS == 1 ? 8 : bit_depth;
  // The short phases of a job -- set-up, work lists, winners: chains of dependent LDS round trips and compares, a few hundred
  // instructions -- run at wave priority 3, the items (thousands of VALU instructions per lane, no waiting) at 0.  A SIMD issues from its
  // oldest ready wave: next to another workgroup's items a short phase got the issue slots those left over and took five times its
  // stand-alone time, half of a job on content whose slots share their motion.  With the priorities the short phases run at their own
  // latency and the items fill every slot they leave, which is nearly all of them.
  __builtin_amdgcn_s_setprio(3);
  // tables that do not depend on the job
  static_assert(9 * (kFracTabH + kFracTabV) <= 152, "me_frac_kernel: the tap tables end where the list counters start");
  if (tid < 9 * kFracTabH) tab_h[tid] = (tid & 7) < 2 * BPS ? me_htap8_dw<BPS>((tid >> 3) / 3, (tid >> 3) % 3, tid & 7) : 0u;
  if (tid >= 128 && tid < 128 + 9 * kFracTabV) {
    const int i = tid - 128, row = i / kFracTabV, j = i - row * kFracTabV;
    tab_v[i] = (float)me_tap8(row / 3, row % 3, j) * (BPS == 1 ? 1.f / 4096.f : __int_as_float((127 - (20 - bd)) << 23));
  }
  for (int i = tid; i < (kFracPairs8 + kFracPairs4) / 8; i += NT) ((uint4*)cover)[i] = ((const uint4*)cover_g)[i];

  // One workgroup per job is the default launch (job_counter == null: workgroup b takes job n_jobs - 1 - b).  With a counter
  // (HMME_FRAC_GRID: fewer workgroups than jobs, each taking job after job as it becomes free) the loop below runs more than once;
  // measured, that launch is the slower one once both deal the jobs last-first.
  uint32_t* next_job = counter + 2;     // LDS word: the job this workgroup works on
#pragma unroll 1
  for (int turn = blockIdx.x;; turn += gridDim.x) {
  int deal = turn;                      // without a counter: blockIdx.x, blockIdx.x + gridDim.x, ...
  if (job_counter) {
    if (tid == 0) *next_job = atomicAdd(job_counter, 1u);
    __syncthreads();                    // (the barrier that ends the previous job's last stage keeps this write behind every read of it)
    deal = (int)*next_job;
  }
  if (deal >= n_jobs || deal < 0) break;
  const int jb = me_frac_deal(deal, n_jobs, prep);
#ifdef ME_FRAC_T_TIMELINE   // timing-only build: when does each job start and end (100 MHz wall clock), in which workgroup, and its phases
  const unsigned long long t_job0 = wall_clock64();
  const unsigned long long c_job0 = clock64();   // shader clock: cycles / wall time = the clock the job ran at
  unsigned long long t_ph[7];   // set-up | per stage: lists, items, winners
  int n_ph = 0;
#define ME_FRAC_STAMP() t_ph[n_ph++] = wall_clock64()
#else
#define ME_FRAC_STAMP()
#endif
  MeJob job;
  if (jobs) {   // a table (job-walking launches, HMME_FRAC_JOB_TABLE, CTU ranges beyond 16 bits), else the job derived here
    job = jobs[jb];
  } else {
    job = me_picture_job(jb, prep.pred_q, nullptr, (int)(prep.ctus & 0xffff), (int)(prep.ctus >> 16), (int)(prep.dims & 0xffff), (int)(prep.dims >> 16), prep.sr);
  }
  const uint8_t* __restrict__ ref_base = refs.base[job.ctu_x & 63];
  const uint8_t* __restrict__ cur_base = curs.base[job.ctu_x & 63];
  job.ctu_x &= ~63;
  const int16_t* mvs = int_mv + (long)jb * kParts * 2;

  // integer MVs outside the CTU's window (not produced by the search) are clamped to it: the patch stays inside the LDS window.
  // One dword per slot (a TComMv), the three loads of a thread in flight together (593 = 2 * 256 + 81)
  {
    static_assert(kParts <= 3 * NT, "slot state set-up assumes three slots per thread");
    const uint32_t* mvw = (const uint32_t*)mvs;
    uint32_t w[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = tid + k * NT < kParts ? mvw[tid + k * NT] : 0u;
    for (int i = tid; i < frac_acc_dw(BPS) / 4; i += NT) ((uint4*)acc)[i] = make_uint4(0, 0, 0, 0);
    const int ltx = job.lt_x, lty = job.lt_y, rbx = job.rb_x, rby = job.rb_y;   // ints: min / max of an int and an int16_t resolve to the double overloads
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (tid + k * NT < kParts) {
        const int mx = min(max((int)(int16_t)(w[k] & 0xffff), ltx), rbx), my = min(max((int)(int16_t)(w[k] >> 16), lty), rby);
        st[tid + k * NT] = (uint32_t)(mx - ltx) | (uint32_t)(my - lty) << 9 | 1u << 18 | 1u << 20;
      }
  }
  if (tid < 2) counter[tid] = 0;
  for (int i = tid; i < 256 * BPS; i += NT) {
    const int r = i / (4 * BPS), q = i - r * (4 * BPS);
    *(uint4*)&curl[r * 16 * BPS + 4 * q] = *(const uint4*)(cur_base + (long)(job.ctu_y + r) * cur_pitch + job.ctu_x * BPS + 16 * q);
  }
  const uint8_t* src = ref_base + (long)(job.ctu_y + job.lt_y - 4) * ref_pitch + (job.ctu_x + job.lt_x - 4) * BPS;   // window sample (-4,-4)
  __syncthreads();
  ME_FRAC_STAMP();

#pragma unroll 1
  for (int stage = 0; stage < 2; ++stage) {
    ME_FRAC_STAMP();   // (timeline builds: the list phase is no phase of its own any more -- its stamp is the stage's start)
    if (stage == 0) me_frac_stage<0, HAD, BPS, WP>(src, ref_pitch, curl, st, cover, list8, list4, counter, pf, tid, bd, clip_lo, wp, tab_h, tab_v, acc);
    else me_frac_stage<1, HAD, BPS, WP>(src, ref_pitch, curl, st, cover, list8, list4, counter, pf, tid, bd, clip_lo, wp, tab_h, tab_v, acc);
    __syncthreads();
    ME_FRAC_STAMP();
    if (tid < 2) counter[tid] = 0;
    // winners (a rolled loop on purpose: with the three slots of a thread unrolled the kernel's register demand rises past 256)
    constexpr int ph[9][2] = {{0, 0}, {0, -1}, {0, 1}, {-1, 0}, {1, 0}, {-1, -1}, {1, -1}, {-1, 1}, {1, 1}};
    constexpr int pq[9][2] = {{0, 0}, {0, -1}, {0, 1}, {-1, -1}, {1, -1}, {-1, 0}, {1, 0}, {-1, 1}, {1, 1}};
#pragma unroll 1
    for (int k = 0; k < 3; ++k) {
      const int s = tid + k * NT;
      if (s >= kParts) break;
      const uint32_t sv = st[s];
      uint32_t sums1[9];
      if constexpr (frac_pack3(BPS)) {
        const unsigned long long* a = (const unsigned long long*)acc + s * 3;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const unsigned long long v = a[q];
          sums1[3 * q] = (uint32_t)v & 0x1fffffu; sums1[3 * q + 1] = (uint32_t)(v >> 21) & 0x1fffffu; sums1[3 * q + 2] = (uint32_t)(v >> 42);
        }
      } else {
#pragma unroll
        for (int i = 0; i < 9; ++i) sums1[i] = acc[s * 9 + i];
      }
      const int mx = (int)(sv & 0x1ff) + job.lt_x, my = (int)((sv >> 9) & 0x1ff) + job.lt_y;
      const int hx = stage ? (int)((sv >> 18) & 3) - 1 : 0, hy = stage ? (int)((sv >> 20) & 3) - 1 : 0;
      const int bxq = 4 * mx + 2 * hx, byq = 4 * my + 2 * hy;   // centre of this stage in quarter units
      uint32_t best = 0xffffffffu, best_acc = 0;
      int bi = 0;
      // the nine points are three x- and three y-offsets: six xGetComponentBits instead of eighteen
      const int step = stage ? 1 : 2;
      uint32_t bits_x[3], bits_y[3];
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        bits_x[t] = me_component_bits(bxq + (t - 1) * step - job.pred_x);
        bits_y[t] = me_component_bits(byq + (t - 1) * step - job.pred_y);
      }
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        // the point orders of the two stages differ in entries 3..6 (s_acMvRefineH / s_acMvRefineQ, TEncSearch.cpp:51-75)
        const uint32_t bx_h = bits_x[ph[i][0] + 1], by_h = bits_y[ph[i][1] + 1], bx_q = bits_x[pq[i][0] + 1], by_q = bits_y[pq[i][1] + 1];
        const uint32_t bits = (ph[i][0] == pq[i][0] && ph[i][1] == pq[i][1]) ? bx_h + by_h : (stage ? bx_q + by_q : bx_h + by_h);
        // whole-PU distortion >> (bitDepth - 8) (TComRdCost.cpp:520-521, :1604), then the MV cost (getCost: uint32 product >> 16)
        const uint32_t a = sums1[i];
        const uint32_t d = (a >> (bd - 8)) + ((lambda_q16 * bits) >> 16);
        if (d < best) { best = d; bi = i; best_acc = a; }
      }
      if (stage == 0) {
        st[s] = (sv & kFracKey0) | (uint32_t)(ph[bi][0] + 1) << 18 | (uint32_t)(ph[bi][1] + 1) << 20;
        // this thread owns row s of acc between the two barriers around this loop: it leaves the row as stage 1 needs it -- point 0 (the
        // centre of the quarter-pel stage IS the half-pel winner: nothing adds to it in stage 1) carried over, the other eight cleared
        if constexpr (frac_pack3(BPS)) {
          unsigned long long* a = (unsigned long long*)acc + s * 3;
          a[0] = best_acc; a[1] = 0; a[2] = 0;
        } else {
          acc[s * 9] = best_acc;
#pragma unroll
          for (int i = 1; i < 9; ++i) acc[s * 9 + i] = 0;
        }
      } else {
        const long o = (long)jb * kParts + s;
        out_qmv[2 * o] = (int16_t)(bxq + pq[bi][0]);
        out_qmv[2 * o + 1] = (int16_t)(byq + pq[bi][1]);
        out_cost[o] = best;
      }
    }
    __syncthreads();   // slot states, cleared sums and list counters are in place before the quarter-pel stage lists its work / the next job starts
    ME_FRAC_STAMP();
  }
#ifdef ME_FRAC_T_TIMELINE
  if (tid == 0) {
    const unsigned long long t1 = wall_clock64();
    uint32_t* o = out_cost + (long)jb * kParts;
    o[0] = (uint32_t)t_job0; o[1] = (uint32_t)(t_job0 >> 32); o[2] = (uint32_t)t1; o[3] = (uint32_t)(t1 >> 32); o[4] = blockIdx.x;
    for (int i = 0; i < 7; ++i) o[5 + i] = (uint32_t)(t_ph[i] - (i ? t_ph[i - 1] : t_job0));   // phase durations, 10 ns units
    o[12] = (uint32_t)(clock64() - c_job0);
  }
  __syncthreads();
#endif
  }   // jobs of this workgroup
}

// ---- explicit weighted prediction on whole pictures (hmme_search_pairs_w_device / hmme_refine_pairs_w_device) ----------------------------
// The picture-sized form of me_weight_window_kernel: a whole padded plane (u8 or u16 samples, margins included) -> a u16 plane of the
// same geometry, every sample ((w0 * v + round) >> shift) + offset_bias (offset_bias = the weight's offset + the bias that keeps block
// and weighted plane unsigned).  Weighting commutes with edge replication, so weighting the margins IS extending the weighted picture.
// The 16-bit search kernel then runs on the result unchanged.  The same kernel makes the other u16 copies a weighted call needs --
// w0 = 1, shift = 0, round = 0 widens (and biases) as it copies: the current pictures' CTU-blocked copies (one "row" of n_ctu * 4096
// samples) and the padded raw copies the weighted refinement reads from 8-bit planes.
// Bandwidth-bound: one lane loads 16 bytes (16 u8 / 8 u16 samples) and stores 16 bytes at a time, rows addressed by pitch (blockIdx.y),
// no division.  cols (samples of a row to convert) is a multiple of 16 and cols * sizeof(SrcT) <= src_pitch, 2 * cols <= dst_pitch:
// every access stays inside its row.
template <typename SrcT>
__global__ void __launch_bounds__(256)
me_weight_plane_kernel(const uint8_t* __restrict__ src, int src_pitch, uint8_t* __restrict__ dst, int dst_pitch, int cols, int w0, int round,
                       int shift, int offset_bias) {
  constexpr int N = 16 / (int)sizeof(SrcT);   // samples per lane
  const long x0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * N;
  if (x0 >= cols) return;
  const uint4 in = *(const uint4*)(src + (long)blockIdx.y * src_pitch + x0 * (long)sizeof(SrcT));
  const uint32_t w[4] = {in.x, in.y, in.z, in.w};
  uint32_t o[N / 2];
#pragma unroll
  for (int i = 0; i < N; i += 2) {
    int v0, v1;
    if (sizeof(SrcT) == 1) { v0 = (int)((w[i >> 2] >> (8 * (i & 3))) & 0xff); v1 = (int)((w[i >> 2] >> (8 * (i & 3) + 8)) & 0xff); }
    else { v0 = (int)(w[i >> 1] & 0xffff); v1 = (int)(w[i >> 1] >> 16); }
    const uint32_t r0 = (uint32_t)(((w0 * v0 + round) >> shift) + offset_bias) & 0xffffu;
    const uint32_t r1 = (uint32_t)(((w0 * v1 + round) >> shift) + offset_bias) & 0xffffu;
    o[i >> 1] = r0 | r1 << 16;
  }
  uint4* out = (uint4*)(dst + (long)blockIdx.y * dst_pitch + x0 * 2);
#pragma unroll
  for (int q = 0; q < N / 8; ++q) out[q] = make_uint4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
}

// ---- motion compensation on whole pictures (hmme_predict_pairs_device) and bi-prediction origins (hmme_search_pairs_bi_device /
// hmme_refine_pairs_bi_device) -------------------------------------------------------------------------------------------------------------
// luma DCT-IF taps by quarter-pel phase (TComInterpolationFilter.cpp:57-63); phase 0 is the copy written as a filter: the two-stage formula
// below then yields the sample itself, which is what HM's filterCopy / single-stage paths produce
__constant__ int kLumaTaps[4][8] = {{0, 0, 0, 64, 0, 0, 0, 0}, {-1, 4, -10, 58, 17, -5, 1, 0}, {-1, 4, -11, 40, 40, -11, 4, -1}, {0, 1, -5, 17, 58, -10, 4, -1}};

// ---- what the three predict kernels share: the constants of a bit depth, the four ends of a sample (HM's "tails"), a block's field
// entry, and the luma sum -----------------------------------------------------------------------------------------------------------------
// the weight of addWeightUni as the kernels take it: round / shift are its round' and shift', made by the host (other_weight_eval)
template <int WP> struct MePredWp {};
template <> struct MePredWp<1> { int w0, round, shift, offset; };
template <> struct MePredWp<2> { MePredWp<1> ref[kMaxRefs]; };

// TComPrediction::xPredInterBlk's shifts and offsets (TComPrediction.cpp:669-707, TComInterpolationFilter.cpp) at one bit depth
struct MePredConst {
  int sh1, off1;   // horizontal pass into the 14-bit intermediate: (sum + off1) >> sh1
  int sh2, off2;   // vertical pass, bi = false: rounds the intermediate back to a sample
  int shb, offb;   // TComYuv::addAvg of two intermediates
  int maxv;        // ClipBD
  __device__ __forceinline__ explicit MePredConst(int bit_depth) {
    const int head = 14 - bit_depth > 2 ? 14 - bit_depth : 2;   // headRoom (IF_INTERNAL_PREC - bitDepth, at least 2)
    sh1 = 6 - head; off1 = -(8192 << sh1);
    sh2 = 6 + head; off2 = (1 << (sh2 - 1)) + (8192 << 6);
    shb = head + 1; offb = (1 << (shb - 1)) + 2 * 8192;
    maxv = (1 << bit_depth) - 1;
  }
};

__device__ __forceinline__ int me_clip_bd(int v, int maxv) { return v < 0 ? 0 : (v > maxv ? maxv : v); }
// xPredInterUni with bi = true leaves the 14-bit intermediate P = sum >> 6 of the vertical pass (shift 6, offset 0, no clip).  HM keeps it in
// a Pel: P + 8192 lies within [-24 576, 40 959] whatever the plane holds, |P| < 2^15.  The reference's own extremes, recorded from its compiled
// filters on the tap-sign pictures of every phase (tests/golden/ref_blocks.npz): luma -25 085 .. 25 079 (12 bit, phase (2, 2)), chroma
// -14 112 .. 14 106 -- the cast never wraps.
__device__ __forceinline__ int me_pel14(int sum) { return (int16_t)(sum >> 6); }

// The four tails take the vertical sum(s) of a sample before any shift and return the sample.
// rounded uni: xPredInterBlk with bi = false (TComPrediction.cpp:590-594, :669): ClipBD((sum + off2) >> sh2), int32 sums -- bit-identical to
// hmo_pred_block_qpel at every phase
__device__ __forceinline__ int me_tail_uni(int sum, const MePredConst& k) { return me_clip_bd((sum + k.off2) >> k.sh2, k.maxv); }
// addWeightUni (TComWeightPrediction.cpp:133-180) in a slice with explicit weighted prediction (TComPrediction::motionCompensation,
// TComPrediction.cpp:527-541): ClipBD(((w0 * (P + 8192) + round') >> shift') + offset), shift' = wp.shift + headRoom, round' = 1 << (shift' - 1).
// The numerator stays inside int32 (hmme_bipred_weight_check); the offset is added in 64 bits, so any int offset is exact before the clip.
// With w0 == 1 << wp.shift and offset 0 this IS me_tail_uni's result (nested floors), which is why identity weights run the unweighted kernels.
__device__ __forceinline__ int me_tail_weight_uni(int sum, const MePredWp<1>& w, int maxv) {
  const long long t = (long long)((w.w0 * (me_pel14(sum) + 8192) + w.round) >> w.shift) + w.offset;
  return t < 0 ? 0 : (t > maxv ? maxv : (int)t);
}
// TComYuv::addAvg (TComYuv.cpp:352-390; TComPrediction.cpp:527-541 without WP): ClipBD((P0 + P1 + offset) >> shift), shift = headRoom + 1,
// offset = (1 << (shift - 1)) + 2 * 8192 -- |P| < 2^15, so int32 holds it at every depth
__device__ __forceinline__ int me_tail_avg(int sum0, int sum1, const MePredConst& k) {
  return me_clip_bd((me_pel14(sum0) + me_pel14(sum1) + k.offb) >> k.shb, k.maxv);
}
// addWeightBi (TComWeightPrediction.cpp:46-49, :67-129; TComPrediction.cpp:603-651 xPredInterBi, :268-301 xWeightedPredictionBi) with the
// bi-directional getWpScaling (:230-247): ClipBD((w0 * (P0 + 8192) + w1 * (P1 + 8192) + add) >> shift), shift = the slice's log2WeightDenom + 1 +
// headRoom, add = (1 << (shift - 1)) + (offset0 + offset1) * 2^(shift - 1) -- the four fields of MePredBiWp<1>, made by the host, which also
// refuses a pair whose numerator could leave int32 (hmme_predict_bi_weight_check), so int32 holds it.  The shift is arithmetic.
__device__ __forceinline__ int me_tail_weight_bi(int sum0, int sum1, int w0, int w1, int add, int shift, int maxv) {
  return me_clip_bd((w0 * (me_pel14(sum0) + 8192) + w1 * (me_pel14(sum1) + 8192) + add) >> shift, maxv);
}

// entry e of a motion field (int16 pairs, quarter-pel luma MVs), clamped like TComDataCU::clipMv for the CTU at luma position (cu_x, cu_y) of a
// pic_w x pic_h luma picture: the patch a block reads then stays within 75 samples of the picture, inside the planes' 128 / 80-sample margins
__device__ __forceinline__ void me_field_mv(const int16_t* __restrict__ mv_field, long e, int cu_x, int cu_y, int pic_w, int pic_h, int& mx, int& my) {
  mx = mv_field[e * 2]; my = mv_field[e * 2 + 1];
  clip_mv_q(mx, my, cu_x, cu_y, pic_w, pic_h);
}

struct MePredCtu { int ctu, cx, cy, cu_x, cu_y; };   // the CTU of a workgroup: its index in the picture, its column and row, its luma position
__device__ __forceinline__ MePredCtu me_pred_ctu(int ctu_first, int pic_w) {
  const int ctus_x = (pic_w + 63) >> 6, ctu = ctu_first + blockIdx.x, cx = ctu % ctus_x, cy = ctu / ctus_x;
  return {ctu, cx, cy, cx * 64, cy * 64};
}

// kLumaTaps for a choice of phase per LANE, in LDS: tap j of a phase = signed byte j of its pair of dwords.  Read behind a barrier.
__device__ __forceinline__ void me_stage_luma_taps(uint32_t (*taps)[2]) {
  if (threadIdx.x < 8) {
    uint32_t p = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) p |= (uint32_t)(uint8_t)kLumaTaps[threadIdx.x >> 1][4 * (threadIdx.x & 1) + j] << (8 * j);
    taps[threadIdx.x >> 1][threadIdx.x & 1] = p;
  }
}

// kMaxRefs weights for a choice per LANE: from the kernel arguments into LDS (int [kMaxRefs * 4]), which keeps the arguments out of scratch;
// read back behind a barrier
__device__ __forceinline__ void me_stage_weights(int* s_weights, const MePredWp<1>* ref) {
  if (threadIdx.x < kMaxRefs * 4) s_weights[threadIdx.x] = ((const int*)ref)[threadIdx.x];
}
__device__ __forceinline__ MePredWp<1> me_staged_weight(const int* s_weights, int i) {
  const int* a = s_weights + 4 * i;   // {w0, round, shift, offset}
  return {a[0], a[1], a[2], a[3]};
}

// the unweighted end of a sample with a direction (use0 || use1): TComYuv::addAvg of both lists, else the rounded sample of the one
__device__ __forceinline__ int me_tail_dir(bool use0, bool use1, int sum0, int sum1, const MePredConst& k) {
  return use0 && use1 ? me_tail_avg(sum0, sum1, k) : me_tail_uni(use0 ? sum0 : sum1, k);
}

// sample v at (x, y) of a pitched image of w x h samples; samples beyond it are not written
template <typename SrcT>
__device__ __forceinline__ void me_store_sample(uint8_t* dst, int pitch, int x, int y, int w, int h, int v) {
  if (x < w && y < h) ((SrcT*)(dst + (long)y * pitch))[x] = (SrcT)v;
}

// the bi-prediction origin 2 * cur - v + bias as u16 (TEncSearch.cpp:3702-3712, TComYuv::removeHighFreq, unclipped) at (x, y) of the CTU whose
// origin block starts at `block`, rows pitch bytes apart; cur from the current picture's CTU-blocked copy
template <typename SrcT>
__device__ __forceinline__ void me_store_origin(const uint8_t* cur_blocks, int ctu, int x, int y, int v, int bias, uint8_t* block, int pitch) {
  const int cur = (int)((const SrcT*)cur_blocks)[(long)ctu * 4096 + y * 64 + x];
  ((uint16_t*)(block + (long)y * pitch))[x] = (uint16_t)(2 * cur - v + bias);
}

// One plane's two passes for the wave's 8x8 luma block at picture position (x0, y0): the 15 x 15 patch at the clamped MV -- rows / columns
// -3 .. +11 around the displaced block -- through LDS (rows of 15 consecutive samples per load), the horizontal pass into the 14-bit
// intermediate (15 rows x 8), the vertical sum of lane (r, c) = (lane >> 3, lane & 7) -- returned before any shift, so that the caller ends it
// with one of the tails.  live is wave-uniform; a wave that is not live reads nothing and still meets both barriers.
template <typename SrcT>
__device__ __forceinline__ int me_predict_block_sum(bool live, const uint8_t* origin, int ref_pitch, int x0, int y0, int mx, int my, int16_t* patch,
                                                    int16_t* mid, int lane, const MePredConst& k) {
  if (live) {
    const uint8_t* src = origin + (long)(y0 + (my >> 2) - 3) * ref_pitch + (long)(x0 + (mx >> 2) - 3) * (long)sizeof(SrcT);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = lane + 64 * j, r = e / 15, c = e - r * 15;
      if (e < 225) patch[r * 16 + c] = (int16_t)((const SrcT*)(src + (long)r * ref_pitch))[c];
    }
  }
  __syncthreads();
  if (live) {
    const int* ch = kLumaTaps[mx & 3];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int o = lane + 64 * j, r = o >> 3, c = o & 7;
      if (o < 120) {
        int sum = 0;
#pragma unroll
        for (int t = 0; t < 8; ++t) sum += ch[t] * (int)patch[r * 16 + c + t];
        mid[o] = (int16_t)((sum + k.off1) >> k.sh1);
      }
    }
  }
  __syncthreads();
  int sum = 0;
  if (live) {
    const int* cv = kLumaTaps[my & 3];
    const int r = lane >> 3, c = lane & 7;
#pragma unroll
    for (int t = 0; t < 8; ++t) sum += cv[t] * (int)mid[(r + t) * 8 + c];
  }
  return sum;
}

// The luma prediction of one CTU per workgroup from a MOTION FIELD: quarter-pel MVs int16 [n_ctu][mv_per_ctu][2], mv_per_ctu = 1 (one MV
// for the CTU: HM's 64x64 2Nx2N) or 64 (one per 8x8 block, raster order inside the CTU), each read through me_field_mv.  A wave takes one
// 8x8 block at a time (16 of the CTU's 64) through me_predict_block_sum.
//   OUT = 0: the prediction, samples of the plane's type, into a pitched image at the block's picture position; samples beyond the
//            picture are not written (blocks wholly outside it are skipped)
//   OUT = 1: the bi-prediction origin 2 * cur - pred + bias as u16 (TEncSearch.cpp:3702-3712, TComYuv::removeHighFreq, unclipped; bias = the
//            pair's: maxv, or more where the searched list's weighted samples go below -maxv), cur from
//            the current picture's CTU-blocked copy -- partial edge CTUs are whole blocks there (edge replication), and so they are here.
//            The block of CTU (cx, cy) starts at dst + cy * dst_ctu_y + cx * dst_ctu_x, its rows dst_pitch bytes apart: the CTU-blocked
//            layout the search reads (8192, ctus_x * 8192, 128) or a padded plane's (128, 64 * pitch, pitch), which the refinement reads
// All stores are 8 consecutive samples per block row.  Bandwidth is not tuned further: the pass moves tens of MB beside a search of
// milliseconds.
//   WP = 0:  me_tail_uni.  Takes an empty struct and compiles to what it did without the argument.
//   WP = 1:  me_tail_weight_uni with the one weight in the kernel arguments (a slice with explicit weighted prediction)
//   REFS = 1: a reference picture per block (hmme_predict_refs_device): ref_field uint8 [n_ctu][mv_per_ctu] names, beside every MV, the
//            plane of `set` the block reads (all of one pitch; ref_origin is not used).  The index is the same for the whole wave -- a
//            wave handles one 8x8 block at a time -- so the choice of the source base is a scalar one.  A block whose index is >= n_refs
//            (0xFF: no CU covers it) is not live: it reads no plane and writes nothing, and still meets both barriers of its iteration.
//            REFS = 0 takes an empty struct and compiles to what it did without it.
//            With OUT = 1 (hmme_search_frame_bi_refs_device: the origin against a reference per block of the other list) every block is
//            written, and an index >= n_refs reads reference 0 -- the blocks outside the picture, whose index is 0xFF and whose MV (0,0).
//   WP = 2:  WP = 1 with one weight per reference picture (hmme_predict_refs_w_device; REFS = 1 only): the block's reference index --
//            already a scalar -- picks its MePredWp<1> among the sixteen in the kernel arguments.  With OUT = 1
//            (hmme_search_frame_bi_refs_w_device) the index is clamped before this lookup, too: an index >= n_refs takes reference 0's weight.
template <int REFS> struct MePredRefs {};
template <> struct MePredRefs<1> { RefSet set; const uint8_t* ref_field; int n_refs; };
template <typename SrcT, int OUT, int WP = 0, int REFS = 0>
__global__ void __launch_bounds__(256)
me_predict_kernel(const uint8_t* __restrict__ ref_origin, int ref_pitch, const int16_t* __restrict__ mv_field, int mv_per_ctu, int ctu_first,
                  int pic_w, int pic_h, int bit_depth, const uint8_t* __restrict__ cur_blocks, int bias, uint8_t* __restrict__ dst,
                  long dst_ctu_x, long dst_ctu_y, int dst_pitch, MePredWp<WP> wp, MePredRefs<REFS> refs) {
  __shared__ int16_t patch[4][15 * 16];
  __shared__ int16_t mid[4][15 * 8];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const auto [ctu, cx, cy, cu_x, cu_y] = me_pred_ctu(ctu_first, pic_w);
  const MePredConst k(bit_depth);
#pragma unroll 1
  for (int it = 0; it < 16; ++it) {
    const int b = it * 4 + wave, bx = (b & 7) * 8, by = (b >> 3) * 8;   // the four waves: four blocks side by side
    const long e = (long)ctu * mv_per_ctu + (mv_per_ctu == 1 ? 0 : b);
    int mx, my;
    me_field_mv(mv_field, e, cu_x, cu_y, pic_w, pic_h, mx, my);
    bool live = OUT == 1 || (cu_x + bx < pic_w && cu_y + by < pic_h);   // wave-uniform
    const uint8_t* origin = ref_origin;
    int ri = 0;
    if constexpr (REFS) {
      ri = __builtin_amdgcn_readfirstlane((int)refs.ref_field[e]);
      if (OUT == 0) live = live && ri < refs.n_refs;   // OUT = 1: every block of the origin is written; such an index reads reference 0
      origin = refs.set.base[ri < refs.n_refs ? ri : 0];
    }
    const int sum = me_predict_block_sum<SrcT>(live, origin, ref_pitch, cu_x + bx, cu_y + by, mx, my, patch[wave], mid[wave], lane, k);
    if (live) {
      const int r = lane >> 3, c = lane & 7;
      int v;
      if constexpr (WP == 2 && OUT == 1) v = me_tail_weight_uni(sum, wp.ref[ri < refs.n_refs ? ri : 0], k.maxv);   // reference 0's plane, and its weight
      else if constexpr (WP == 2) v = me_tail_weight_uni(sum, wp.ref[ri], k.maxv);   // live: ri < n_refs
      else if constexpr (WP == 1) v = me_tail_weight_uni(sum, wp, k.maxv);
      else v = me_tail_uni(sum, k);
      if (OUT == 0) me_store_sample<SrcT>(dst, dst_pitch, cu_x + bx + c, cu_y + by + r, pic_w, pic_h, v);
      else me_store_origin<SrcT>(cur_blocks, ctu, bx + c, by + r, v, bias, dst + cy * dst_ctu_y + cx * dst_ctu_x, dst_pitch);
    }
  }
}

// ---- the luma prediction from one MV per 4x4 block (hmme_predict_refs4_device; the rule: include/hmme.h) ---------------------------------
// me_predict_kernel<SrcT, 0, WP, 1> with HM's own motion storage: mv_field int16 [n_ctu][256][2], ref_field uint8 [n_ctu][256] (null: every
// block index 0), entry b the 4x4 block at ((b & 15) * 4, (b >> 4) * 4) of the CTU.  One CTU per workgroup of four waves, a wave one 8x8
// block at a time, lane (r, c) = (lane >> 3, lane & 7) one sample -- but the block is four QUADRANTS, lane (r, c) in quadrant
// (r >> 2) * 2 + (c >> 2), each with its own entry: its own clamped MV (me_field_mv: the CTU's clamp, so the sample is the one the 64 form
// writes when the 8x8 block carries this entry), its own plane, its own weight.
//
// me_predict4_pass is one list's pass for the wave's 8x8 block at picture position (x0, y0), and the only place that stages, filters and sums
// quadrants (me_predict4_kernel: one pass per iteration; me_predict_bi4_kernel: list 0's, then list 1's).  live, mx, my are the LANE's -- those
// of its quadrant, equal in the quadrant's 16 lanes; plane_of(from) is the plane of the quadrant whose first lane is `from`, wave-uniform.
// Returns the vertical sum of lane (r, c) before any shift (0 in a lane that is not live), which the caller ends with one of the tails.
//   stage       per quadrant the 11 x 11 patch at its MV -- rows / columns -3 .. +7 around the displaced 4x4 block, a subset of the 15 x 15
//               patch the 64 form reads at that MV, so the planes' margins hold -- into wave-private LDS: four patches of 11 rows, pitch 12.
//               Quadrant by quadrant, so MV, plane and liveness of a load are scalars (readlane of the quadrant's first lane).
//   horizontal  the 14-bit intermediate, 11 rows x 4 columns per quadrant, 176 outputs per wave in three steps; the taps are chosen per
//               lane by the output's quadrant (me_stage_luma_taps)
//   vertical    lane (r, c): eight rows of its quadrant's intermediate with the taps of its own vertical phase
// Pitch 12, not 11: rows stay dword-aligned and a quadrant's patch starts 66 dwords after the one before, two banks further; with either
// pitch the 8 rows x 4 lanes of a half-wave's u16 reads span more than 32 banks and wrap once.  Measured: a pitch of 11 gives the same
// times within 1 % (profiles/predict4_patch_pitch_ab.txt).
// BARRIER INVARIANT (of every kernel that calls this pass or me_predict_chroma4_pass): __syncthreads() is a barrier of the whole workgroup.
// Every wave and every 16-lane group -- live, partly live or wholly dead -- runs all iterations of its kernel's loop and meets the same two
// barriers in each pass: stage | barrier | horizontal | barrier | vertical.  Everything that depends on the field (liveness, direction, the
// plane, the phase) sits INSIDE a stage; no barrier is ever inside a branch, a pass is never called inside one, and no wave leaves the loop
// early.
template <typename SrcT, class PlaneOf>
__device__ __forceinline__ int me_predict4_pass(bool live, PlaneOf plane_of, int ref_pitch, int x0, int y0, int mx, int my, int16_t* wpatch, int16_t* wmid,
                                                const uint32_t (*taps)[2], int lane, const MePredConst& k) {
  const int r = lane >> 3, c = lane & 7, q = (r >> 2) * 2 + (c >> 2);
  int info[4];   // scalars: 4 | horizontal phase of a live quadrant, else 0
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int from = (s >> 1) * 32 + (s & 1) * 4;
    const int s_live = __builtin_amdgcn_readlane((int)live, from), s_mx = __builtin_amdgcn_readlane(mx, from), s_my = __builtin_amdgcn_readlane(my, from);
    info[s] = s_live ? 4 | (s_mx & 3) : 0;
    if (s_live) {
      const uint8_t* src = plane_of(from) + (long)(y0 + (s >> 1) * 4 + (s_my >> 2) - 3) * ref_pitch + (long)(x0 + (s & 1) * 4 + (s_mx >> 2) - 3) * (long)sizeof(SrcT);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int el = lane + 64 * j, pr = el / 11, pc = el - pr * 11;
        if (el < 121) wpatch[s * 132 + pr * 12 + pc] = (int16_t)((const SrcT*)(src + (long)pr * ref_pitch))[pc];
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int o = lane + 64 * j, oq = o / 44, rem = o - oq * 44;   // output (row rem >> 2, column rem & 3) of quadrant oq
    const int inf = oq == 0 ? info[0] : (oq == 1 ? info[1] : (oq == 2 ? info[2] : info[3]));
    if (o < 176 && inf) {
      const uint32_t lo = taps[inf & 3][0], hi = taps[inf & 3][1];
      const int16_t* p = wpatch + oq * 132 + (rem >> 2) * 12 + (rem & 3);
      int sum = 0;
#pragma unroll
      for (int t = 0; t < 4; ++t) sum += (int)(int8_t)(lo >> (8 * t)) * (int)p[t] + (int)(int8_t)(hi >> (8 * t)) * (int)p[t + 4];
      wmid[o] = (int16_t)((sum + k.off1) >> k.sh1);
    }
  }
  __syncthreads();
  int sum = 0;
  if (live) {
    const uint32_t lo = taps[my & 3][0], hi = taps[my & 3][1];
    const int16_t* p = wmid + q * 44 + (r & 3) * 4 + (c & 3);
#pragma unroll
    for (int t = 0; t < 4; ++t) sum += (int)(int8_t)(lo >> (8 * t)) * (int)p[4 * t] + (int)(int8_t)(hi >> (8 * t)) * (int)p[4 * (t + 4)];
  }
  return sum;
}

// me_predict4_kernel: one pass per iteration, the plane of a quadrant being set.base[its index]; the tail is me_tail_uni (WP = 0) or
// me_tail_weight_uni with the weight of the lane's reference (WP = 2).  Index and weight are per lane, not per wave: me_stage_weights.
// A quadrant is live if its 4x4 block starts inside the picture and its index is < n_refs; one that is not reads no plane and its lanes
// write nothing.  The barrier invariant is the pass's: the loop has 16 iterations for every wave.
//   OUT = 0: the prediction, as described above.  Takes an empty MePred4Origin and compiles to what it did without the parameter.
//   OUT = 1: the bi-prediction origin 2 * cur - pred + bias as u16 from a 4x4 field (hmme_search_pairs_bi4_device / hmme_refine_pairs_bi4_device;
//            WP = 0 only, n_refs = 1 with a null ref_field; hmme_search_frame_bi_refs4_device / hmme_refine_frame_bi_refs4_device: the other
//            list's set, count and reference field, an index >= n_refs -- 0xFF beyond the picture edge -- clamped to 0 per lane before the
//            readlane plane lookup, so that every quadrant reads a plane of the set), as me_predict_kernel<SrcT, 1> forms it from a 64 field:
//            EVERY quadrant is live, those beyond the picture edge included, cur comes from the current picture's CTU-blocked copy, and the
//            block of CTU (cx, cy) starts at dst + cy * ctu_y + cx * ctu_x with rows dst_pitch bytes apart (the search's CTU blocks or the
//            refinement's padded plane).  Liveness no longer depends on the field, so the barrier invariant holds as it did.
template <int OUT> struct MePred4Origin {};
template <> struct MePred4Origin<1> { const uint8_t* cur_blocks; int bias; long ctu_x, ctu_y; };
template <typename SrcT, int WP, int OUT = 0>
__global__ void __launch_bounds__(256)
me_predict4_kernel(RefSet set, int n_refs, int ref_pitch, const int16_t* __restrict__ mv_field, const uint8_t* __restrict__ ref_field, int ctu_first,
                   int pic_w, int pic_h, int bit_depth, uint8_t* __restrict__ dst, int dst_pitch, MePredWp<WP> wp, MePred4Origin<OUT> org) {
  static_assert(WP == 0 || WP == 2, "one weight per reference, or none");
  static_assert(OUT == 0 || WP == 0, "the origin from a 4x4 field is unweighted");
  __shared__ int16_t patch[4][4 * 11 * 12];
  __shared__ int16_t mid[4][4 * 11 * 4];
  __shared__ uint32_t taps[4][2];
  __shared__ int s_weights[kMaxRefs * 4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  me_stage_luma_taps(taps);
  if constexpr (WP == 2) me_stage_weights(s_weights, wp.ref);
  const auto [ctu, cx, cy, cu_x, cu_y] = me_pred_ctu(ctu_first, pic_w);
  const MePredConst k(bit_depth);
  const int r = lane >> 3, c = lane & 7;
#pragma unroll 1
  for (int it = 0; it < 16; ++it) {
    const int b = it * 4 + wave, bx = (b & 7) * 8, by = (b >> 3) * 8;   // the four waves: four 8x8 blocks side by side
    const int qx = bx + (c & 4), qy = by + (r & 4);                      // this lane's 4x4 block inside the CTU
    const long e = (long)ctu * 256 + (qy >> 2) * 16 + (qx >> 2);
    int ri = ref_field ? (int)ref_field[e] : 0;
    if (OUT == 1 && ri >= n_refs) ri = 0;   // every block of an origin is written; such an index reads reference 0
    const bool live = OUT == 1 || (cu_x + qx < pic_w && cu_y + qy < pic_h && ri < n_refs);
    int mx = 0, my = 0;
    if (live) me_field_mv(mv_field, e, cu_x, cu_y, pic_w, pic_h, mx, my);
    else ri = 0;
    const auto plane_of = [&](int from) { return set.base[__builtin_amdgcn_readlane(ri, from)]; };
    const int sum = me_predict4_pass<SrcT>(live, plane_of, ref_pitch, cu_x + bx, cu_y + by, mx, my, patch[wave], mid[wave], taps, lane, k);
    if (live) {
      int v;
      if constexpr (WP == 2) v = me_tail_weight_uni(sum, me_staged_weight(s_weights, ri), k.maxv);
      else v = me_tail_uni(sum, k);
      if constexpr (OUT == 0) me_store_sample<SrcT>(dst, dst_pitch, cu_x + bx + c, cu_y + by + r, pic_w, pic_h, v);
      else me_store_origin<SrcT>(org.cur_blocks, ctu, bx + c, by + r, v, org.bias, dst + cy * org.ctu_y + cx * org.ctu_x, dst_pitch);
    }
  }
}

// ---- partition decision and motion field from the 593-slot tables (hmme_select_pairs_device; the rule: include/hmme.h) ------------------
// hmme_select_params as the kernel takes it
struct MeSelect {
  int per;                  // mv_per_ctu: 64 | 256
  int mv_unit, price_mv;
  uint32_t part_mask;
  int min_depth, max_depth;
  uint32_t cu_cost, pu_cost;
};

// slot of a PU: the closed form of TComDataCU::getIndexBlock the host uses (hmme.hip slot_of); D = depth, (cx, cy) = the CU at that depth.
// The caller never asks for AMP at depth 3.
template <int D>
__device__ __forceinline__ int me_slot_of(int ps, int idx, int cx, int cy) {
  constexpr int n = 1 << D;
  constexpr int b2Nx2N = D == 0 ? 592 : D == 1 ? 584 : D == 2 ? 544 : 384, b2NxN = D == 0 ? 588 : D == 1 ? 560 : D == 2 ? 448 : 0;
  constexpr int bNx2N = D == 0 ? 590 : D == 1 ? 568 : D == 2 ? 480 : 128, bAMP = D == 0 ? 576 : D == 1 ? 512 : 256;
  const int r = cy * n + cx;
  if (ps == 0) return b2Nx2N + r;
  if (ps == 1) return b2NxN + cy * 2 * n + idx * n + cx;
  if (ps == 2) return bNx2N + cy * 2 * n + 2 * cx + idx;
  const int k = ps == 4 ? (idx ? 3 : 0) : ps == 5 ? (idx ? 1 : 2) : ps == 6 ? (idx ? 7 : 4) : (idx ? 5 : 6);   // 2NxnU, 2NxnD, nLx2N, nRx2N
  return bAMP + k * n * n + r;
}
// may PartSize ps be coded for a CU of depth D?  AMP is not tabulated at 8x8; with one MV per 8x8 block every PU rectangle must be 8-aligned
template <int D>
__device__ __forceinline__ bool me_select_allowed(const MeSelect& a, int ps) {
  if (!((a.part_mask >> ps) & 1u)) return false;
  if (D == 3) return ps == 0 || (ps <= 2 && a.per == 256);
  if (D == 2) return ps <= 2 || a.per == 256;
  return true;
}
// slot of the PU of a depth-D CU with PartSize ps that covers sample (x, y) of the CTU
template <int D>
__device__ __forceinline__ int me_select_pu_slot(int ps, int x, int y) {
  constexpr int s = 64 >> D;
  const int lx = x & (s - 1), ly = y & (s - 1);
  const int idx = ps == 0 ? 0 : ps == 1 ? ly >= s / 2 : ps == 2 ? lx >= s / 2 : ps == 4 ? ly >= s / 4 : ps == 5 ? ly >= 3 * s / 4 : ps == 6 ? lx >= s / 4 : lx >= 3 * s / 4;
  return me_slot_of<D>(ps, idx, x >> (6 - D), y >> (6 - D));
}
__device__ __forceinline__ int me_select_pu_slot_at(int depth, int ps, int x, int y) {
  return depth == 0 ? me_select_pu_slot<0>(ps, x, y) : depth == 1 ? me_select_pu_slot<1>(ps, x, y) : depth == 2 ? me_select_pu_slot<2>(ps, x, y) : me_select_pu_slot<3>(ps, x, y);
}
__device__ __forceinline__ uint64_t me_shfl_xor_u64(uint64_t v, int mask) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, mask), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), mask);
  return (uint64_t)hi << 32 | lo;
}
// The prices the select kernels put on an MV dword (x in the low half), each defined here once.
// HM's MV cost of a table entry, for the callers that set price_mv (mv_unit: the table holds integer pels)
__device__ __forceinline__ uint32_t me_select_mv_price(const MeSelect& a, uint32_t lambda_q16, uint32_t m, int pred_x, int pred_y) {
  const int vx = (int16_t)(m & 0xffffu), vy = (int16_t)(m >> 16);
  return a.mv_unit ? me_mv_cost(lambda_q16, vx, vy, pred_x, pred_y) : me_mv_cost_q(lambda_q16, vx, vy, pred_x, pred_y);
}
// HM's getBits at cost scale 0 of a quarter-pel MV against its predictor
__device__ __forceinline__ uint32_t me_select_mv_bits(uint32_t m, int pred_x, int pred_y) {
  return me_component_bits((int16_t)(m & 0xffffu) - pred_x) + me_component_bits((int16_t)(m >> 16) - pred_y);
}
// TComRdCost::getCost: the product wraps in 32 bits
__device__ __forceinline__ uint64_t me_select_get_cost(uint32_t lambda_q16, uint32_t bits) { return (lambda_q16 * bits) >> 16; }
// a refinement table's cost with the MV cost of `bits` taken out again, clamped at 0: the distortion
__device__ __forceinline__ uint64_t me_select_dist(uint32_t lambda_q16, uint32_t cost, uint32_t bits) {
  const uint64_t g = me_select_get_cost(lambda_q16, bits);
  return cost > g ? cost - g : 0;
}

// what the decision carries for one lane (= one 8x8 block): the resolved cost of the lane's ancestor CU at the depth handled last (the same
// value in every lane of that CU) and the shallowest ancestor that stayed a leaf so far
struct MeSelectState {
  uint64_t resolved;
  int leaf_depth, leaf_ps;   // leaf_depth < 0: no CU covers the block
};

// One level of the bottom-up decision, for the lane's ancestor CU at depth D.  Every lane of the CU computes the CU's own best redundantly
// (LDS broadcast reads, no divergence), the sum of the four children is a quad reduction over the lanes that differ in bit (2 - D) of the
// block's column and row.  Called for D = 3, 2, 1, 0: a shallower leaf overrides a deeper one, so no decision has to be pushed back down.
// CostT: the element type of the slot costs -- uint32_t table costs (me_select_kernel) or the 64-bit merged costs of me_select_refs_kernel.
template <int D, typename CostT>
__device__ __forceinline__ void me_select_level(const MeSelect& a, const CostT* s_cost, const uint32_t* s_mv, uint32_t lambda_q16, int pred_x, int pred_y,
                                                int bx, int by, int ctu_x, int ctu_y, int pic_w, int pic_h, MeSelectState& st) {
  if (D > a.max_depth) return;   // wave-uniform
  constexpr int s = 64 >> D;
  const int cx = bx >> (3 - D), cy = by >> (3 - D), x0 = ctu_x + cx * s, y0 = ctu_y + cy * s;
  auto pu = [&](int slot) -> uint64_t {   // slot cost (+ HM's MV cost) + pu_cost
    uint64_t c = (uint64_t)s_cost[slot] + a.pu_cost;
    if (a.price_mv) c += me_select_mv_price(a, lambda_q16, s_mv[slot], pred_x, pred_y);
    return c;
  };
  uint64_t own = a.cu_cost + pu(me_slot_of<D>(0, 0, cx, cy));   // bit 0 of part_mask is always set
  int own_ps = 0;
#pragma unroll
  for (int ps = 1; ps < 8; ++ps) {
    if (ps == 3 || (D == 3 && ps > 2)) continue;
    if (!me_select_allowed<D>(a, ps)) continue;   // wave-uniform
    const uint64_t c = a.cu_cost + pu(me_slot_of<D>(ps, 0, cx, cy)) + pu(me_slot_of<D>(ps, 1, cx, cy));
    if (c < own) { own = c; own_ps = ps; }   // strict: the lower enum wins ties
  }
  if (D == a.max_depth) {   // exists if and only if its origin lies inside the picture
    const bool exists = x0 < pic_w && y0 < pic_h;
    st.resolved = exists ? own : 0;
    if (exists) { st.leaf_depth = D; st.leaf_ps = own_ps; }
    return;
  }
  uint64_t children = st.resolved + me_shfl_xor_u64(st.resolved, 1 << (2 - D));
  children += me_shfl_xor_u64(children, 8 << (2 - D));
  const bool may_leaf = D >= a.min_depth && x0 + s <= pic_w && y0 + s <= pic_h;
  if (may_leaf && !(children < own)) { st.resolved = own; st.leaf_depth = D; st.leaf_ps = own_ps; }   // the parent wins ties
  else st.resolved = children;
}

// What the four select kernels share.  Their geometry: one wave per CTU, four CTUs per workgroup, blockIdx.y = picture (pair); lane = 8x8
// block in RASTER order inside the CTU -- the layout of the field, so that every store of the wave is one contiguous run.  Each kernel is
// me_select_wave, its own merge of the tables into the CTU's slots in LDS, a barrier, and me_select_decide_store.
struct MeSelectWave {
  int wave, lane;    // of the workgroup
  int c, ctu, pic;   // the CTU's index in the tables (which begin at ctu_first) and in the picture; the picture (pair) of the launch
  bool live;         // wave-uniform: the CTU lies inside the range
};
__device__ __forceinline__ MeSelectWave me_select_wave(int ctu_first, int ctu_count) {
  MeSelectWave w;
  w.wave = threadIdx.x >> 6; w.lane = threadIdx.x & 63;
  w.c = blockIdx.x * 4 + w.wave; w.ctu = ctu_first + w.c; w.pic = blockIdx.y;
  w.live = w.c < ctu_count;
  return w;
}

// what is decided: one table set per picture pair (me_select_kernel), the reference per PU (me_select_refs_kernel), L0 / L1 / bi per PU
// (me_select_dirs_kernel) and that with a reference index per list (me_select_dirs_refs_kernel)
enum MeSelectMode { kSelTable, kSelRefs, kSelDirs, kSelDirsRefs };

// what a kernel's merge leaves in LDS per slot of the wave's CTU.  A member no mode of the kernel uses is null and never looked at
template <typename CostT>
struct MeSelectSlots {
  CostT* cost;     // kSelTable: the table's cost (uint32_t).  Every other mode: the winner's cost in 64 bits, priced -- the MV cost is inside
  uint32_t* mv;    // the table's / the winner's MV dword
  uint8_t* ref;    // kSelRefs: the winner's reference index
  uint8_t* dir;    // kSelDirs, kSelDirsRefs: the winner's direction (1, 2, 3) | the list the bi pass searched << 2
  uint8_t* lref;   // kSelDirsRefs: the winner's reference index in list 0 and, kParts + 3 bytes on, in list 1; 0xFF in a list the winner does not use
};
// where the outputs go, and the inputs that are copied into them.  Per picture of the launch a field is [n_ctu][per] dwords, or with two
// lists [2][n_ctu][64]; references are laid out like the field with bytes for dwords; null where the mode (or the caller: slot, cost) has none
struct MeSelectOut {
  uint32_t* field;             // the motion field; kSelDirs, kSelDirsRefs: two lists -- the winner's MV in its list, in the other list (0,0)
                               // under a direction-1 / -2 slot and the block's own entry of uni_field under a direction-3 slot
  uint16_t* slot;              // the covering slot per block, 0xFFFF where no CU covers it
  uint32_t* cost;              // the CTU's cost, saturated
  uint8_t* ref;                // kSelRefs: the reference index per block; kSelDirsRefs: per list, travelling with the MV (else 0xFF / uni_ref's)
  uint8_t* dir;                // kSelDirs, kSelDirsRefs: the direction per block, 0xFF where no CU covers it
  const uint32_t* uni_field;   // kSelDirs, kSelDirsRefs: the lists' fields of the uni-directional decisions, laid out like field
  const uint8_t* uni_ref;      // kSelDirsRefs: their reference indices, laid out like ref
};

// The decision over the CTU's slots in LDS and the stores that follow it: what every select kernel ends in.  Outside kSelTable the MV cost
// is inside the merged cost already -- against each reference's own predictor -- and is not priced a second time.
// FOUR (kSelDirs, kSelDirsRefs): the caller is me_select_dirs_kernel<true> or me_select_dirs_refs_kernel<true>, whose a.per is 256 -- the
// direction stores of the 256 layout (with kSelDirsRefs: and the per-list reference bytes, as paired 16-bit stores beside the uint2 field
// stores) exist in those instantiations alone, so that every other one keeps the instructions it had.
template <MeSelectMode MODE, typename CostT, bool FOUR = false>
__device__ __forceinline__ void me_select_decide_store(const MeSelect& params, const MeSelectSlots<CostT>& s, const MeSelectOut& out, const MeSelectWave& w,
                                                       uint32_t lambda_q16, int pred_x, int pred_y, int pic_w, int pic_h, int n_ctu) {
  constexpr bool REFS = MODE == kSelRefs, DIRS = MODE == kSelDirs || MODE == kSelDirsRefs, LREFS = MODE == kSelDirsRefs;
  MeSelect a = params;
  if (MODE != kSelTable) a.price_mv = 0;
  const int lane = w.lane, bx = lane & 7, by = lane >> 3, ctus_x = (pic_w + 63) >> 6;
  const int ctu_x = (w.ctu % ctus_x) * 64, ctu_y = (w.ctu / ctus_x) * 64;
  const long o = (long)w.pic * n_ctu + w.ctu;   // the CTU's index in the outputs
  MeSelectState st = {0, -1, 0};
  me_select_level<3>(a, s.cost, s.mv, lambda_q16, pred_x, pred_y, bx, by, ctu_x, ctu_y, pic_w, pic_h, st);
  me_select_level<2>(a, s.cost, s.mv, lambda_q16, pred_x, pred_y, bx, by, ctu_x, ctu_y, pic_w, pic_h, st);
  me_select_level<1>(a, s.cost, s.mv, lambda_q16, pred_x, pred_y, bx, by, ctu_x, ctu_y, pic_w, pic_h, st);
  me_select_level<0>(a, s.cost, s.mv, lambda_q16, pred_x, pred_y, bx, by, ctu_x, ctu_y, pic_w, pic_h, st);
  if (lane == 0 && out.cost) out.cost[o] = st.resolved > 0xffffffffull ? 0xffffffffu : (uint32_t)st.resolved;
  // integer-pel MVs leave as quarter pels: both halves of the dword << 2, the two bits that cross into the upper half masked off
  auto field_mv = [&](int slot) -> uint32_t {
    const uint32_t m = s.mv[slot];
    return a.mv_unit ? (m << 2) & 0xfffcfffcu : m;
  };
  static_assert(!FOUR || DIRS, "the direction stores of the 256 layout: a B-picture decision");
  if (!FOUR && a.per == 64) {
    const int slot = st.leaf_depth < 0 ? 0xffff : me_select_pu_slot_at(st.leaf_depth, st.leaf_ps, bx * 8, by * 8);
    if constexpr (DIRS) {   // (one MV per 4x4 block: the kSelDirs branch further down)
      const long lists = (long)n_ctu * 64, e = 2 * w.pic * lists + w.ctu * 64 + lane;   // the block in list 0 of its picture; list 1: `lists` further
      const int d = slot == 0xffff ? 0 : (int)s.dir[slot];
      const int dir = d & 3, bl = d >> 2;
      uint32_t f[2] = {0u, 0u};
      if (dir == 3) { f[bl] = s.mv[slot]; f[1 - bl] = out.uni_field[e + (1 - bl) * lists]; }
      else if (dir) f[dir - 1] = s.mv[slot];
      out.field[e] = f[0];
      out.field[e + lists] = f[1];
      out.dir[o * 64 + lane] = dir ? (uint8_t)dir : (uint8_t)0xff;
      if constexpr (LREFS) {
        uint8_t rl[2] = {0xff, 0xff};
        if (dir == 3) { rl[bl] = s.lref[bl * (kParts + 3) + slot]; rl[1 - bl] = out.uni_ref[e + (1 - bl) * lists]; }
        else if (dir) rl[dir - 1] = s.lref[(dir - 1) * (kParts + 3) + slot];
        out.ref[e] = rl[0];
        out.ref[e + lists] = rl[1];
      }
    } else {
      out.field[o * 64 + lane] = slot == 0xffff ? 0u : field_mv(slot);
      if constexpr (REFS) out.ref[o * 64 + lane] = slot == 0xffff ? (uint8_t)0xff : s.ref[slot];
    }
    if (out.slot) out.slot[o * 64 + lane] = (uint16_t)slot;
  } else {
#pragma unroll
    for (int j = 0; j < 2; ++j) {   // the block's two rows of two 4x4 blocks
      int slot[2];
      uint32_t mv[2], ref[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        slot[i] = st.leaf_depth < 0 ? 0xffff : me_select_pu_slot_at(st.leaf_depth, st.leaf_ps, bx * 8 + 4 * i, by * 8 + 4 * j);
        mv[i] = slot[i] == 0xffff ? 0u : field_mv(slot[i]);
        if constexpr (REFS) ref[i] = slot[i] == 0xffff ? 0xffu : (uint32_t)s.ref[slot[i]];
      }
      const long e = o * 256 + (2 * by + j) * 16 + 2 * bx;   // even: 8-byte (MVs) / 4-byte (slots) / 2-byte (references, directions) aligned pairs
      if constexpr (FOUR) {   // hmme_select_dirs4_device, hmme_select_dirs_refs4_device: the 64 branch above per 4x4 block, with the paired stores of REFS
        const long lists = (long)n_ctu * 256, e0 = 2 * w.pic * lists + (long)w.ctu * 256 + (2 * by + j) * 16 + 2 * bx;   // the pair in list 0 of its picture
        uint32_t f[2][2], dirs[2];
        [[maybe_unused]] uint32_t rl[2][2];   // LREFS: the reference index of each list
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int d = slot[i] == 0xffff ? 0 : (int)s.dir[slot[i]];
          const int dir = d & 3, bl = d >> 2;
          // the winner's list: the one a bi candidate searched, else the direction's; under direction 3 the other list holds the 4x4
          // block's own entry of uni_field (a 4-byte aligned input: one dword per block), else (0,0)
          const int wl = dir == 3 ? bl : dir - 1;
          const uint32_t other = dir == 3 ? out.uni_field[e0 + i + (1 - bl) * lists] : 0u;
          f[0][i] = wl == 0 ? mv[i] : other;
          f[1][i] = wl == 1 ? mv[i] : other;
          dirs[i] = dir ? (uint32_t)dir : 0xffu;
          if constexpr (LREFS) {   // hmme_select_dirs_refs4_device: the indices travel with the MVs -- the block's own entry of uni_ref, else 0xFF
            const uint32_t own = dir ? (uint32_t)s.lref[wl * (kParts + 3) + slot[i]] : 0xffu;
            const uint32_t other_ref = dir == 3 ? (uint32_t)out.uni_ref[e0 + i + (1 - bl) * lists] : 0xffu;
            rl[0][i] = wl == 0 ? own : other_ref;
            rl[1][i] = wl == 1 ? own : other_ref;
          }
        }
        *(uint2*)(out.field + e0) = make_uint2(f[0][0], f[0][1]);
        *(uint2*)(out.field + e0 + lists) = make_uint2(f[1][0], f[1][1]);
        *(uint16_t*)(out.dir + e) = (uint16_t)(dirs[0] | dirs[1] << 8);
        if constexpr (LREFS) {
          *(uint16_t*)(out.ref + e0) = (uint16_t)(rl[0][0] | rl[0][1] << 8);
          *(uint16_t*)(out.ref + e0 + lists) = (uint16_t)(rl[1][0] | rl[1][1] << 8);
        }
      } else {
        *(uint2*)(out.field + e) = make_uint2(mv[0], mv[1]);
      }
      if constexpr (REFS) *(uint16_t*)(out.ref + e) = (uint16_t)(ref[0] | ref[1] << 8);
      if (out.slot) *(uint32_t*)(out.slot + e) = (uint32_t)slot[0] | (uint32_t)slot[1] << 16;
    }
  }
}

// The merge: the CTU's 593 costs and MVs loaded coalesced into LDS (4.7 KB per CTU).  mv_tab: int16 [n_pairs][ctu_count][593][2] read as
// dwords; cost_tab: uint32 [n_pairs][ctu_count][593]; pred_q: int16 [n_pairs][n_ctu][2] or null; out_field: int16 [n_pairs][n_ctu][per][2]
// written as dwords (256 B of MVs per wave with one MV per 8x8 block; rows of 64 B with four); out_slot: uint16 [n_pairs][n_ctu][per] or
// null; out_cost: uint32 [n_pairs][n_ctu] or null.  Bandwidth-sized: nothing tuned beyond coalesced accesses.
__global__ void __launch_bounds__(256)
me_select_kernel(const uint32_t* __restrict__ mv_tab, const uint32_t* __restrict__ cost_tab, const int16_t* __restrict__ pred_q,
                 uint32_t* __restrict__ out_field, uint16_t* __restrict__ out_slot, uint32_t* __restrict__ out_cost, MeSelect a, int pic_w, int pic_h,
                 int n_ctu, int ctu_first, int ctu_count, uint32_t lambda_q16) {
  __shared__ uint32_t s_cost[4][kParts + 3];
  __shared__ uint32_t s_mv[4][kParts + 3];
  const MeSelectWave w = me_select_wave(ctu_first, ctu_count);
  if (w.live) {
    const long base = ((long)w.pic * ctu_count + w.c) * kParts;
    for (int i = w.lane; i < kParts; i += 64) {
      s_cost[w.wave][i] = cost_tab[base + i];
      s_mv[w.wave][i] = mv_tab[base + i];
    }
  }
  __syncthreads();
  if (!w.live) return;
  const long o = (long)w.pic * n_ctu + w.ctu;
  const int pred_x = pred_q ? pred_q[o * 2] : 0, pred_y = pred_q ? pred_q[o * 2 + 1] : 0;
  me_select_decide_store<kSelTable, uint32_t>(a, {s_cost[w.wave], s_mv[w.wave]}, {out_field, out_slot, out_cost}, w, lambda_q16, pred_x, pred_y, pic_w, pic_h,
                                              n_ctu);
}

// ---- reference picture per PU (hmme_select_refs_device; the rule: include/hmme.h) --------------------------------------------------------
// the caller's price of each reference index, as the kernel takes it
struct MeRefCost { uint32_t c[kMaxRefs]; };

// me_select_kernel with a reference dimension in front.  The tables are those of one multi-reference launch -- mv_tab int16
// [n_pics][n_refs][ctu_count][593][2] as dwords, cost_tab uint32 of the same shape, pred_q int16 [n_pics][n_refs][n_ctu][2] or null.  The
// merge: a lane owns the slots lane, lane + 64, ... (ten, the last one in 17 lanes only) and walks the references with coalesced loads
// straight from the tables, its slots' running best -- the priced cost in 64 bits, the MV dword, the reference -- in registers: no LDS
// traffic, no atomic and no cross-lane step in the reference loop; the predictor and the price of a reference are wave-uniform.  The
// comparison is strict in the order 0, 1, ...: the lowest index wins ties (TEncSearch.cpp:3086).  Behind the last reference the merged slots
// go to LDS (7.6 KB per CTU with the costs in 64 bits: unsaturated).  out_ref: uint8 [n_pics][n_ctu][per], a wave's bytes one run of 64
// with one MV per 8x8 block, pairs of them as one 16-bit store with four.  Bandwidth-sized like its sibling: n_refs x 7.1 KB in per CTU,
// under 2 KB out.
__global__ void __launch_bounds__(256)
me_select_refs_kernel(const uint32_t* __restrict__ mv_tab, const uint32_t* __restrict__ cost_tab, const int16_t* __restrict__ pred_q,
                      uint32_t* __restrict__ out_field, uint8_t* __restrict__ out_ref, uint16_t* __restrict__ out_slot, uint32_t* __restrict__ out_cost,
                      MeSelect a, MeRefCost ref_cost, int n_refs, int pic_w, int pic_h, int n_ctu, int ctu_first, int ctu_count, uint32_t lambda_q16) {
  constexpr int kOwn = (kParts + 63) / 64;   // slots per lane
  __shared__ uint64_t s_cost[4][kParts + 3];
  __shared__ uint32_t s_mv[4][kParts + 3];
  __shared__ uint8_t s_ref[4][kParts + 3];
  const MeSelectWave w = me_select_wave(ctu_first, ctu_count);
  if (w.live) {
    uint64_t best[kOwn];
    uint32_t best_mv[kOwn];
    int best_ref[kOwn];
#pragma unroll 1
    for (int r = 0; r < n_refs; ++r) {
      const long set = (long)w.pic * n_refs + r, base = (set * ctu_count + w.c) * kParts, po = (set * n_ctu + w.ctu) * 2;
      const int pred_x = pred_q ? pred_q[po] : 0, pred_y = pred_q ? pred_q[po + 1] : 0;
      const uint32_t rc = ref_cost.c[r];
#pragma unroll
      for (int k = 0; k < kOwn; ++k) {
        const int i = w.lane + 64 * k;
        if (i >= kParts) continue;
        const uint32_t m = mv_tab[base + i];
        uint64_t p = (uint64_t)cost_tab[base + i] + rc;
        if (a.price_mv) p += me_select_mv_price(a, lambda_q16, m, pred_x, pred_y);
        if (r == 0 || p < best[k]) { best[k] = p; best_mv[k] = m; best_ref[k] = r; }   // strict: the lower index wins ties
      }
    }
#pragma unroll
    for (int k = 0; k < kOwn; ++k) {
      const int i = w.lane + 64 * k;
      if (i >= kParts) continue;
      s_cost[w.wave][i] = best[k];
      s_mv[w.wave][i] = best_mv[k];
      s_ref[w.wave][i] = (uint8_t)best_ref[k];
    }
  }
  __syncthreads();
  if (!w.live) return;
  me_select_decide_store<kSelRefs, uint64_t>(a, {s_cost[w.wave], s_mv[w.wave], s_ref[w.wave]}, {out_field, out_slot, out_cost, out_ref}, w, lambda_q16, 0, 0, pic_w,
                                             pic_h, n_ctu);
}

// ---- L0, L1 or bi per PU, with one reference per list (hmme_select_dirs_device) or several (hmme_select_dirs_refs_device; the rule of
// each: include/hmme.h) ----------------------------------------------------------------------------------------------------------------------
// hmme_dir_params / hmme_dir_refs_params of every picture of the launch, as the kernels take them
constexpr int kMaxDirRefs = 8;
struct MeDirBits { uint32_t dir_bits[3], list_bits[2]; };
struct MeDirParams { MeDirBits p[4]; };
struct MeDirRefsBits { uint32_t dir_bits[3]; int n_refs[2]; uint32_t ref_bits[2][kMaxDirRefs]; uint32_t l1_valid_mask; };
struct MeDirRefsParams { MeDirRefsBits p[4]; };

// One reference per list: FOUR table sets per picture -- uni / bi, each int16 [n_pics][2][ctu_count][593][2] as dwords with costs uint32 of
// that shape; pred_q int16 [n_pics][2][n_ctu][2] or null.  The merge: a lane takes each of its slots (lane, lane + 64, ...) through the four
// sets in registers, all eight loads up front: the distortions with the MV cost taken out again (the bi pass's halved: fWeight 0.5,
// TEncSearch.cpp:3808), HM's bits put back in ONE getCost per candidate, every sum in 64 bits.  The bi candidate is list 0's unless list 1's
// is strictly cheaper (:3183-3186, :3226); bi wins on <= against both lists, list 0 on <= against list 1 (:3291, :3314).  This is the
// sibling's merge at one reference per list, written out: as one body with it, it measured 15 % slower.
// uni_field / out_field: int16 [n_pics][2][n_ctu][64][2] as dwords; out_dir uint8 [n_pics][n_ctu][64].
//   FOUR = false: one MV per 8x8 block (hmme_select_dirs_device); the instructions it had before the parameter existed.
//   FOUR = true:  one MV per 4x4 block (hmme_select_dirs4_device; a.per == 256, fields and directions [..][256]).  All 593 slots take part,
//                 so TComDataCU::isBipredRestriction (TComDataCU.cpp:2892-2904, tested at TEncSearch.cpp:3109) applies: the 8x4 / 4x8 PUs of
//                 an 8x8 CU -- depth 3, PartSize 1 or 2: slots 0..255 (me_slot_of<3>) -- form no bi candidate.  Their bi tables are not even
//                 loaded, so what those entries hold cannot reach an output.
template <bool FOUR>
__global__ void __launch_bounds__(256)
me_select_dirs_kernel(const uint32_t* __restrict__ mv_uni, const uint32_t* __restrict__ cost_uni, const uint32_t* __restrict__ mv_bi,
                      const uint32_t* __restrict__ cost_bi, const uint32_t* __restrict__ uni_field, const int16_t* __restrict__ pred_q,
                      uint32_t* __restrict__ out_field, uint8_t* __restrict__ out_dir, uint16_t* __restrict__ out_slot, uint32_t* __restrict__ out_cost,
                      MeSelect a, MeDirParams dirs, int pic_w, int pic_h, int n_ctu, int ctu_first, int ctu_count, uint32_t lambda_q16) {
  constexpr int kOwn = (kParts + 63) / 64;   // slots per lane
  __shared__ uint64_t s_cost[4][kParts + 3];
  __shared__ uint32_t s_mv[4][kParts + 3];
  __shared__ uint8_t s_dir[4][kParts + 3];
  const MeSelectWave w = me_select_wave(ctu_first, ctu_count);
  if (w.live) {
    const MeDirBits b = dirs.p[w.pic];
    int px[2] = {0, 0}, py[2] = {0, 0};
    if (pred_q) {   // wave-uniform: the two lists' predictors of the CTU
      const int16_t* pq = pred_q + ((long)w.pic * 2 * n_ctu + w.ctu) * 2;
      px[0] = pq[0]; py[0] = pq[1];
      px[1] = pq[2 * (long)n_ctu]; py[1] = pq[2 * (long)n_ctu + 1];
    }
    const long base[2] = {((long)w.pic * 2 * ctu_count + w.c) * kParts, (((long)w.pic * 2 + 1) * ctu_count + w.c) * kParts};
#pragma unroll 1
    for (int k = 0; k < kOwn; ++k) {
      const int i = w.lane + 64 * k;
      if (i >= kParts) continue;
      uint32_t mu[2], mb[2], bu[2], bb[2];
      uint64_t cu[2], cb[2];
      const bool may_bi = !FOUR || i >= 256;   // FOUR: isBipredRestriction for the slots of 8x4 / 4x8 PUs (wave-uniform: k < 4)
#pragma unroll
      for (int l = 0; l < 2; ++l) {
        mu[l] = mv_uni[base[l] + i];
        mb[l] = may_bi ? mv_bi[base[l] + i] : 0u;
        bu[l] = me_select_mv_bits(mu[l], px[l], py[l]);
        bb[l] = me_select_mv_bits(mb[l], px[l], py[l]);
      }
#pragma unroll
      for (int l = 0; l < 2; ++l) {
        cu[l] = me_select_dist(lambda_q16, cost_uni[base[l] + i], bu[l]) + me_select_get_cost(lambda_q16, b.dir_bits[l] + b.list_bits[l] + bu[l]);
        cb[l] = (me_select_dist(lambda_q16, may_bi ? cost_bi[base[l] + i] : 0u, bb[l]) >> 1) +
                me_select_get_cost(lambda_q16, b.dir_bits[2] + b.list_bits[0] + b.list_bits[1] + bb[l] + bu[1 - l]);
      }
      const int bl = cb[1] < cb[0] ? 1 : 0;   // strict: list 0 is tried first
      const uint64_t cbi = cb[bl];
      uint64_t best;
      uint32_t m;
      int d;
      if (may_bi && cbi <= cu[0] && cbi <= cu[1]) { best = cbi; m = mb[bl]; d = 3 | bl << 2; }
      else if (cu[0] <= cu[1]) { best = cu[0]; m = mu[0]; d = 1; }
      else { best = cu[1]; m = mu[1]; d = 2; }
      s_cost[w.wave][i] = best;
      s_mv[w.wave][i] = m;
      s_dir[w.wave][i] = (uint8_t)d;
    }
  }
  __syncthreads();
  if (!w.live) return;
  me_select_decide_store<kSelDirs, uint64_t, FOUR>(a, {s_cost[w.wave], s_mv[w.wave], nullptr, s_dir[w.wave]}, {out_field, out_slot, out_cost, nullptr, out_dir, uni_field},
                                                   w, lambda_q16, 0, 0, pic_w, pic_h, n_ctu);
}

// Up to eight references per list: me_select_dirs_kernel with a reference dimension behind the list -- uni / bi tables int16
// [n_pics][2][R][ctu_count][593][2] as dwords with costs uint32 of that shape, pred_q int16 [n_pics][2][R][n_ctu][2] or null (R =
// n_refs_max); list l uses its first n_refs[l] sets.  The merge walks each of a lane's slots through the references of both lists in
// registers, twice: the uni pass keeps per list the first strict minimum (:3086) with its MV, index and motion bits (ref_bits + MV bits,
// :3154-3155), list 1 also the minimum over the references of l1_valid_mask -- its direction-2 candidate (:3096-3104, :3282-3285), absent
// with an empty mask; the bi pass prices every reference against the OTHER list's motion bits (:3210-3219) and keeps the first strict
// minimum (:3226).  Predictors and bit counts are wave-uniform; no LDS traffic, no atomic and no cross-lane step in the reference loops.
// The two reference indices per slot go to LDS on top of the sibling's (35.8 KB per workgroup).  uni_ref / out_ref: uint8
// [n_pics][2][n_ctu][64] beside the fields.
//   FOUR = false: one MV per 8x8 block (hmme_select_dirs_refs_device); the instructions it had before the parameter existed.
//   FOUR = true:  one MV per 4x4 block (hmme_select_dirs_refs4_device; a.per == 256, fields, reference bytes and directions [..][256]).  All
//                 593 slots take part, so TComDataCU::isBipredRestriction (TComDataCU.cpp:2892-2904, tested at TEncSearch.cpp:3109) applies
//                 as in me_select_dirs_kernel<true>: slots 0..255 form no bi candidate for any reference -- the bi pass over the references
//                 is not run for them (wave-uniform: k < 4), so their bi tables are not loaded -- and decide between list 0's best and list
//                 1's direction-2 candidate alone.  The LDS is the 64 form's.
template <bool FOUR = false>
__global__ void __launch_bounds__(256)
me_select_dirs_refs_kernel(const uint32_t* __restrict__ mv_uni, const uint32_t* __restrict__ cost_uni, const uint32_t* __restrict__ mv_bi,
                           const uint32_t* __restrict__ cost_bi, const uint32_t* __restrict__ uni_field, const uint8_t* __restrict__ uni_ref,
                           const int16_t* __restrict__ pred_q, uint32_t* __restrict__ out_field, uint8_t* __restrict__ out_ref, uint8_t* __restrict__ out_dir,
                           uint16_t* __restrict__ out_slot, uint32_t* __restrict__ out_cost, MeSelect a, MeDirRefsParams dirs, int n_refs_max, int pic_w,
                           int pic_h, int n_ctu, int ctu_first, int ctu_count, uint32_t lambda_q16) {
  constexpr int kOwn = (kParts + 63) / 64;   // slots per lane
  __shared__ uint64_t s_cost[4][kParts + 3];
  __shared__ uint32_t s_mv[4][kParts + 3];
  __shared__ uint8_t s_dir[4][kParts + 3];
  __shared__ uint8_t s_lref[4][2 * (kParts + 3)];
  const MeSelectWave w = me_select_wave(ctu_first, ctu_count);
  if (w.live) {
    const MeDirRefsBits& b = dirs.p[w.pic];
    // set (l, r) of the picture: its table row of this CTU, its predictor of this CTU (wave-uniform)
    auto row = [&](int l, int r) -> long { return ((((long)w.pic * 2 + l) * n_refs_max + r) * ctu_count + w.c) * kParts; };
    auto pred = [&](int l, int r, int& px, int& py) {
      px = 0; py = 0;
      if (pred_q) {
        const int16_t* pq = pred_q + ((((long)w.pic * 2 + l) * n_refs_max + r) * n_ctu + w.ctu) * 2;
        px = pq[0]; py = pq[1];
      }
    };
#pragma unroll 1
    for (int k = 0; k < kOwn; ++k) {
      const int i = w.lane + 64 * k;
      if (i >= kParts) continue;
      uint64_t cu[2] = {0, 0}, cb[2] = {0, 0}, cv = 0;   // cv: list 1's direction-2 candidate
      uint32_t mu[2] = {0, 0}, mb[2] = {0, 0}, mot[2] = {0, 0}, mvv = 0;
      int ru[2] = {0, 0}, rb[2] = {0, 0}, rv = -1;   // rv < 0: no reference of the mask yet
#pragma unroll
      for (int l = 0; l < 2; ++l) {
#pragma unroll 1
        for (int r = 0; r < b.n_refs[l]; ++r) {
          int px, py;
          pred(l, r, px, py);
          const long at = row(l, r) + i;
          const uint32_t m = mv_uni[at], bits = me_select_mv_bits(m, px, py);
          const uint64_t p = me_select_dist(lambda_q16, cost_uni[at], bits) + me_select_get_cost(lambda_q16, b.dir_bits[l] + b.ref_bits[l][r] + bits);
          if (r == 0 || p < cu[l]) { cu[l] = p; mu[l] = m; ru[l] = r; mot[l] = b.ref_bits[l][r] + bits; }   // strict: the lower index wins ties
          if (l == 1 && ((b.l1_valid_mask >> r) & 1u) && (rv < 0 || p < cv)) { cv = p; mvv = m; rv = r; }
        }
      }
      const bool may_bi = !FOUR || i >= 256;   // FOUR: isBipredRestriction for the slots of 8x4 / 4x8 PUs (wave-uniform: k < 4)
#pragma unroll
      for (int l = 0; l < 2; ++l) {
#pragma unroll 1
        for (int r = 0; may_bi && r < b.n_refs[l]; ++r) {
          int px, py;
          pred(l, r, px, py);
          const long at = row(l, r) + i;
          const uint32_t m = mv_bi[at], bits = me_select_mv_bits(m, px, py);
          const uint64_t p = (me_select_dist(lambda_q16, cost_bi[at], bits) >> 1) + me_select_get_cost(lambda_q16, b.dir_bits[2] + b.ref_bits[l][r] + bits + mot[1 - l]);
          if (r == 0 || p < cb[l]) { cb[l] = p; mb[l] = m; rb[l] = r; }
        }
      }
      const int bl = cb[1] < cb[0] ? 1 : 0;   // strict: list 0 is tried first
      const uint64_t cbi = cb[bl];
      uint64_t best;
      uint32_t m;
      int d, r0 = 0xff, r1 = 0xff;
      if (may_bi && cbi <= cu[0] && (rv < 0 || cbi <= cv)) { best = cbi; m = mb[bl]; d = 3 | bl << 2; r0 = rb[0]; r1 = rb[1]; }
      else if (rv < 0 || cu[0] <= cv) { best = cu[0]; m = mu[0]; d = 1; r0 = ru[0]; }
      else { best = cv; m = mvv; d = 2; r1 = rv; }
      s_cost[w.wave][i] = best;
      s_mv[w.wave][i] = m;
      s_dir[w.wave][i] = (uint8_t)d;
      s_lref[w.wave][i] = (uint8_t)r0;
      s_lref[w.wave][kParts + 3 + i] = (uint8_t)r1;
    }
  }
  __syncthreads();
  if (!w.live) return;
  me_select_decide_store<kSelDirsRefs, uint64_t, FOUR>(a, {s_cost[w.wave], s_mv[w.wave], nullptr, s_dir[w.wave], s_lref[w.wave]},
                                                 {out_field, out_slot, out_cost, out_ref, out_dir, uni_field, uni_ref}, w, lambda_q16, 0, 0, pic_w, pic_h, n_ctu);
}

// ---- residual and per-PU / per-CU distortion of a prediction (hmme_residual_pairs_device; the rule: include/hmme.h) -----------------------
// The slot layout read backwards: what me_slot_of<D> encodes, by the bases of its families.  Depth of the CU a slot belongs to:
//   [0, 256) 2NxN / Nx2N of 8x8 CUs, [256, 384) AMP of 16x16, [384, 448) 2Nx2N 8x8, [448, 512) 2NxN / Nx2N 16x16, [512, 544) AMP 32x32,
//   [544, 560) 2Nx2N 16x16, [560, 576) 2NxN / Nx2N 32x32, [576, 584) AMP 64x64, [584, 588) 2Nx2N 32x32, [588, 593) the 64x64 CU's other shapes
__host__ __device__ constexpr int me_slot_depth(int s) {
  return s < 256 ? 3 : s < 384 ? 2 : s < 448 ? 3 : s < 512 ? 2 : s < 544 ? 1 : s < 560 ? 2 : s < 576 ? 1 : s < 584 ? 0 : s < 588 ? 1 : 0;
}
// xGetHADs takes 8x8 Hadamards when both sides of the PU are multiples of 8: everything but 8x4 / 4x8 (slots 0..255) and the AMP shapes of a
// 16x16 CU (16x4, 16x12, 4x16, 12x16: slots 256..383).  Such a PU is 8-aligned in position as well, so it covers whole lane quads.
__host__ __device__ constexpr bool me_slot_had8(int s) { return s >= 384; }
// index of the depth-d CU that holds the 4x4 block (bx4, by4) among the CTU's 85 CUs: 1 + 4 + 16 + 64, raster order inside a depth
__host__ __device__ constexpr int me_cu_index(int depth, int bx4, int by4) {
  return ((1 << (2 * depth)) - 1) / 3 + ((by4 >> (4 - depth)) << depth) + (bx4 >> (4 - depth));
}
constexpr int kResidualCus = 85;
static_assert(me_cu_index(3, 15, 15) == kResidualCus - 1 && me_cu_index(0, 15, 15) == 0 && me_cu_index(1, 8, 0) == 2 && me_cu_index(2, 0, 4) == 9, "85 CUs per CTU");
static_assert(me_slot_depth(0) == 3 && me_slot_depth(255) == 3 && me_slot_depth(256) == 2 && me_slot_depth(383) == 2 && me_slot_depth(384) == 3 &&
              me_slot_depth(447) == 3 && me_slot_depth(448) == 2 && me_slot_depth(511) == 2 && me_slot_depth(512) == 1 && me_slot_depth(543) == 1 &&
              me_slot_depth(544) == 2 && me_slot_depth(559) == 2 && me_slot_depth(560) == 1 && me_slot_depth(575) == 1 && me_slot_depth(576) == 0 &&
              me_slot_depth(583) == 0 && me_slot_depth(584) == 1 && me_slot_depth(587) == 1 && me_slot_depth(588) == 0 && me_slot_depth(592) == 0,
              "the family bases of me_slot_of");

// the int16 residual images of a launch, one per pair (null: the pair has none)
struct MeResidualSet { uint8_t* base[kMaxRefs]; };

__device__ __forceinline__ int me_quad_xor1(int v) { return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false); }   // quad_perm [1,0,3,2]
__device__ __forceinline__ int me_quad_xor2(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false); }   // quad_perm [2,3,0,1]
__device__ __forceinline__ uint32_t me_quad_sum(uint32_t v) {
  v += (uint32_t)me_quad_xor1((int)v);
  return v + (uint32_t)me_quad_xor2((int)v);
}
__device__ __forceinline__ uint32_t me_wave_sum(uint32_t v) {
#pragma unroll
  for (int m = 32; m; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m);
  return v;
}
// one row of four samples, widened; the address is 4-byte aligned
template <typename SrcT>
__device__ __forceinline__ void me_load_row4(const uint8_t* p, int* v) {
  if (sizeof(SrcT) == 1) {
    const uint32_t a = *(const uint32_t*)p;
    v[0] = a & 0xff; v[1] = (a >> 8) & 0xff; v[2] = (a >> 16) & 0xff; v[3] = a >> 24;
  } else {
    const uint32_t a = ((const uint32_t*)p)[0], b = ((const uint32_t*)p)[1];
    v[0] = a & 0xffff; v[1] = a >> 16; v[2] = b & 0xffff; v[3] = b >> 16;
  }
}
// the unnormalised 4-point Walsh-Hadamard butterfly on v[0], v[s], v[2s], v[3s]
__device__ __forceinline__ void me_wht4(int* v, int s) {
  const int s0 = v[0] + v[s], s1 = v[0] - v[s], s2 = v[2 * s] + v[3 * s], s3 = v[2 * s] - v[3 * s];
  v[0] = s0 + s2; v[s] = s1 + s3; v[2 * s] = s0 - s2; v[3 * s] = s1 - s3;
}

// One workgroup of 256 lanes per CTU, blockIdx.y = pair; a lane holds one 4x4 block.  Lanes 4q .. 4q + 3 hold the four 4x4 blocks of 8x8
// block q (raster order inside the CTU), so an 8x8 block is one DPP quad: its Hadamard is the 2x2 butterfly over the quad's four 4x4
// transforms (H8 = H2 (x) H4: the |coefficients| are a permutation of xCalcHADs8x8's, the sum is the same), two quad_perm moves per
// coefficient and no LDS, as me_frac_kernel assembles its own.  The 16 current samples come from the plane's CTU-blocked copy (whole for
// partial CTUs), the 16 predicted ones from the pair's image: whole rows of four where the block lies inside the picture and the pitch is a
// multiple of 4, sample by sample otherwise; a sample outside the picture has difference 0 and is never read from the image.  SAD, SSE and
// the 4x4 transform are exact 32-bit integers in the lane.
//   MAP:  slot_map (uint16 [n_pairs][n_ctu][PER]) names the PU of every block.  Per-PU and per-CU sums are ds_add_u32 into two LDS tables
//         (593 slots, 85 CUs); one lane of a quad adds the 8x8 value of a slot made of 8x8 Hadamards.  After a barrier every lane reads its
//         slot's and its CU's total.  A slot >= 593 (0xFFFF: no CU covers the block) carries 0 and adds nothing.
//   !MAP: every block (8x8 with PER 64, 4x4 with 256) is its own PU and CU: no tables.
// out_pu / out_cu: uint32 [n_pairs][n_ctu][PER]; out_ctu: uint32 [n_pairs][n_ctu][2] = (sum of the PU errors, sum of the CU SSEs); each may
// be null.  With PER 64 lane 0 of a quad stores its block; a wave's stores are one run of 64 B (PER 64) or 256 B.  The residual leaves as
// 8-byte rows, only inside the picture.  No scratch.  Bandwidth-sized: nothing tuned beyond that.
template <typename SrcT, int PER, bool HAD, bool MAP>
__global__ void __launch_bounds__(256)
me_residual_kernel(RefSet cur_blocks, RefSet preds, int pred_pitch, const uint16_t* __restrict__ slot_map, MeResidualSet resid, int resid_pitch,
                   uint32_t* __restrict__ out_pu, uint32_t* __restrict__ out_cu, uint32_t* __restrict__ out_ctu, int pic_w, int pic_h, int bit_depth,
                   int n_ctu, int ctu_first) {
  __shared__ uint32_t s_pu[MAP ? kParts + 3 : 1];
  __shared__ uint32_t s_cu[MAP ? kResidualCus + 3 : 1];
  __shared__ uint32_t s_tot[2];
  const int tid = threadIdx.x, q = tid >> 2, sub = tid & 3;
  const int bx4 = 2 * (q & 7) + (sub & 1), by4 = 2 * (q >> 3) + (sub >> 1);
  const int pair = blockIdx.y, ctu = ctu_first + blockIdx.x, ctus_x = (pic_w + 63) >> 6;
  const int x0 = (ctu % ctus_x) * 64 + bx4 * 4, y0 = (ctu / ctus_x) * 64 + by4 * 4;
  const long o = (long)pair * n_ctu + ctu;
  if constexpr (MAP) {
    for (int i = tid; i < kParts; i += 256) s_pu[i] = 0;
    if (tid < kResidualCus) s_cu[tid] = 0;
  }
  if (tid < 2) s_tot[tid] = 0;

  // the lane's 16 differences
  int d[16];
  const uint8_t* cb = cur_blocks.base[pair] + ((long)ctu * 4096 + by4 * 256 + bx4 * 4) * (long)sizeof(SrcT);
  const uint8_t* pb = preds.base[pair] + (long)y0 * pred_pitch + (long)x0 * (long)sizeof(SrcT);
  const bool whole = x0 + 4 <= pic_w && y0 + 4 <= pic_h;
  const bool rows4 = whole && !(pred_pitch & 3);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int c[4], p[4];
    me_load_row4<SrcT>(cb + r * 64 * (int)sizeof(SrcT), c);
    if (rows4) {
      me_load_row4<SrcT>(pb + (long)r * pred_pitch, p);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        p[i] = (x0 + i < pic_w && y0 + r < pic_h) ? (int)((const SrcT*)(pb + (long)r * pred_pitch))[i] : c[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) d[4 * r + i] = c[i] - p[i];
  }
  uint8_t* rb = resid.base[pair];   // workgroup-uniform
  if (rb) {
    rb += (long)y0 * resid_pitch + (long)x0 * 2;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (whole) {
        *(uint2*)(rb + (long)r * resid_pitch) = make_uint2((uint32_t)(d[4 * r] & 0xffff) | (uint32_t)d[4 * r + 1] << 16,
                                                           (uint32_t)(d[4 * r + 2] & 0xffff) | (uint32_t)d[4 * r + 3] << 16);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (x0 + i < pic_w && y0 + r < pic_h) ((int16_t*)(rb + (long)r * resid_pitch))[i] = (int16_t)d[4 * r + i];
      }
    }
  }

  // SAD, SSE (xGetSSE: every square shifted before it is added) and, with HAD, the 4x4 and the quad's 8x8 Hadamard sums
  const int sh = bit_depth - 8;
  uint32_t sad = 0, sse = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    sad += (uint32_t)(d[i] < 0 ? -d[i] : d[i]);
    sse += (uint32_t)(d[i] * d[i]) >> (sh << 1);
  }
  uint32_t e4 = sad, e8 = 0;   // the block's PU error before the PU's shift: alone, and (lanes of a quad alike) as a quarter of its 8x8 block
  if constexpr (HAD) {
#pragma unroll
    for (int r = 0; r < 4; ++r) me_wht4(d + 4 * r, 1);
#pragma unroll
    for (int c = 0; c < 4; ++c) me_wht4(d + c, 4);
    uint32_t a4 = 0, a8 = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      a4 += (uint32_t)(d[i] < 0 ? -d[i] : d[i]);
      const int n1 = me_quad_xor1(d[i]);
      const int t = (sub & 1) ? n1 - d[i] : d[i] + n1;
      const int n2 = me_quad_xor2(t);
      const int u = (sub & 2) ? n2 - t : t + n2;
      a8 += (uint32_t)(u < 0 ? -u : u);
    }
    e4 = (a4 + 1) >> 1;                 // xCalcHADs4x4
    e8 = (me_quad_sum(a8) + 2) >> 2;    // xCalcHADs8x8
  } else {
    e8 = me_quad_sum(sad);
  }

  uint32_t pu, cu, t_pu, t_cu;   // what the lane's block carries; what the lane adds to the CTU's two sums
  bool store;
  long at;
  if (PER == 64) { store = sub == 0; at = o * 64 + q; } else { store = true; at = o * 256 + by4 * 16 + bx4; }
  if constexpr (MAP) {
    const int s = slot_map[at];          // with PER 64 the quad's four lanes read the same entry
    const bool valid = s < kParts;
    const int ci = me_cu_index(me_slot_depth(s), bx4, by4);
    __syncthreads();                     // the tables are zero
    if (valid) {
      const uint32_t add = !HAD ? sad : me_slot_had8(s) ? (sub == 0 ? e8 : 0u) : e4;
      if (add) atomicAdd(&s_pu[s], add);
      if (sse) atomicAdd(&s_cu[ci], sse);
    }
    __syncthreads();
    pu = valid ? s_pu[s] >> sh : 0u;
    cu = valid ? s_cu[ci] : 0u;
    t_pu = 0;
    for (int i = tid; i < kParts; i += 256) t_pu += s_pu[i] >> sh;
    t_cu = tid < kResidualCus ? s_cu[tid] : 0u;
  } else {
    pu = (PER == 64 ? e8 : e4) >> sh;
    cu = PER == 64 ? me_quad_sum(sse) : sse;
    t_pu = store ? pu : 0u;
    t_cu = store ? cu : 0u;
    __syncthreads();                     // s_tot is zero
  }
  if (store) {
    if (out_pu) out_pu[at] = pu;
    if (out_cu) out_cu[at] = cu;
  }
  if (out_ctu) {   // workgroup-uniform
    t_pu = me_wave_sum(t_pu);
    t_cu = me_wave_sum(t_cu);
    if ((tid & 63) == 0) { atomicAdd(&s_tot[0], t_pu); atomicAdd(&s_tot[1], t_cu); }
    __syncthreads();
    if (tid < 2) out_ctu[o * 2 + tid] = s_tot[tid];
  }
}

// ---- the prediction of a picture whose blocks are L0, L1 or bi (hmme_predict_bi_device) ----------------------------------------------------
// me_predict_kernel<SrcT, 0> with a direction per block: one CTU per workgroup, a wave one 8x8 block at a time.  mv_field: int16
// [2][n_ctu][mv_per_ctu][2] (list-major), dir_field: uint8 [n_ctu][mv_per_ctu] -- HM's interDir: 1 = list 0 (ref0), 2 = list 1 (ref1),
// 3 = both.  The direction is the same for the whole wave, so it is read as a scalar; a list the direction does not name is not live in its
// pass of me_predict_block_sum.  Any direction outside 1..3 (0xFF: no CU) reads no plane and writes nothing, and still meets all four
// barriers of its iteration.
//   WP = 0:  direction 1 / 2: me_tail_uni, the sample me_predict_kernel writes from that plane and MV; direction 3: me_tail_avg.  Takes an
//            empty struct and compiles to what it did without the argument.
//   WP = 1:  the same picture in a B slice with getWPBiPred() (hmme_predict_bi_w_device).  Direction 1 / 2: me_tail_weight_uni with that
//            list's weight (uni[]); direction 3: me_tail_weight_bi.
//   REFS = 1: a reference picture per block and list (hmme_predict_bi_refs_device; WP = 0 only): ref_field uint8 [2][n_ctu][mv_per_ctu]
//            (list-major, like the MVs) names the plane of set[l] a block reads in list l (all of one pitch; ref0 / ref1 are not used).
//            Both indices are wave-uniform like the direction, so the source bases are scalar choices, each clamped before the lookup.  A
//            block that uses a list whose index is >= n[l] (0xFF: no CU) is like a block without a direction: it reads no plane and
//            writes nothing.  The index of a list the direction does not name is not looked at.  REFS = 0 takes an empty struct and
//            compiles to what it did without it.
//   WP = 2:  WP = 1 with one weight per reference picture and list (hmme_predict_bi_refs_w_device; REFS = 1 only).  Both indices are already
//            scalars, so ref[l][index] is a scalar load of kernel arguments, clamped like the plane base: a block that is not live never
//            indexes beyond its list.  Direction 1 / 2: me_tail_weight_uni with ref[l][r].  Direction 3: me_tail_weight_bi with the two
//            entries' w0, the slice's common shift' = log2WeightDenom + 1 + headRoom and add = (1 + offset0 + offset1) * 2^(shift' - 1),
//            formed here -- the host has checked every (r0, r1) pair's numerator against int32.
template <int WP> struct MePredBiWp {};
template <> struct MePredBiWp<1> { int w0, w1, add, shift; MePredWp<1> uni[2]; };
template <> struct MePredBiWp<2> { MePredWp<1> ref[2][kMaxRefs]; int shift; };
template <int REFS> struct MePredBiRefs {};
template <> struct MePredBiRefs<1> { RefSet set[2]; const uint8_t* ref_field; int n[2]; };
template <typename SrcT, int WP = 0, int REFS = 0>
__global__ void __launch_bounds__(256)
me_predict_bi_kernel(const uint8_t* __restrict__ ref0, const uint8_t* __restrict__ ref1, int ref_pitch, const int16_t* __restrict__ mv_field,
                     const uint8_t* __restrict__ dir_field, int mv_per_ctu, int n_ctu, int ctu_first, int pic_w, int pic_h, int bit_depth,
                     uint8_t* __restrict__ dst, int dst_pitch, MePredBiWp<WP> wp, MePredBiRefs<REFS> refs) {
  __shared__ int16_t patch[4][15 * 16];
  __shared__ int16_t mid[4][15 * 8];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const auto [ctu, cx, cy, cu_x, cu_y] = me_pred_ctu(ctu_first, pic_w);
  const MePredConst k(bit_depth);
#pragma unroll 1
  for (int it = 0; it < 16; ++it) {
    const int b = it * 4 + wave, bx = (b & 7) * 8, by = (b >> 3) * 8;   // the four waves: four blocks side by side
    const long e = (long)ctu * mv_per_ctu + (mv_per_ctu == 1 ? 0 : b);
    const int dir = __builtin_amdgcn_readfirstlane((int)dir_field[e]);
    bool in_pic = cu_x + bx < pic_w && cu_y + by < pic_h && dir >= 1 && dir <= 3;   // wave-uniform
    const uint8_t* origin0 = ref0;
    const uint8_t* origin1 = ref1;
    int i0 = 0, i1 = 0;   // WP = 2: the clamped indices
    if constexpr (REFS) {
      const int r0 = __builtin_amdgcn_readfirstlane((int)refs.ref_field[e]);
      const int r1 = __builtin_amdgcn_readfirstlane((int)refs.ref_field[(long)n_ctu * mv_per_ctu + e]);
      in_pic = in_pic && (!(dir & 1) || r0 < refs.n[0]) && (!(dir & 2) || r1 < refs.n[1]);
      origin0 = refs.set[0].base[r0 < refs.n[0] ? r0 : 0];
      origin1 = refs.set[1].base[r1 < refs.n[1] ? r1 : 0];
      if constexpr (WP == 2) { i0 = r0 < refs.n[0] ? r0 : 0; i1 = r1 < refs.n[1] ? r1 : 0; }
    }
    const bool use0 = in_pic && (dir & 1), use1 = in_pic && (dir & 2);
    int mx0 = 0, my0 = 0, mx1 = 0, my1 = 0;
    if (use0) me_field_mv(mv_field, e, cu_x, cu_y, pic_w, pic_h, mx0, my0);
    if (use1) me_field_mv(mv_field, (long)n_ctu * mv_per_ctu + e, cu_x, cu_y, pic_w, pic_h, mx1, my1);
    const int sum0 = me_predict_block_sum<SrcT>(use0, origin0, ref_pitch, cu_x + bx, cu_y + by, mx0, my0, patch[wave], mid[wave], lane, k);
    const int sum1 = me_predict_block_sum<SrcT>(use1, origin1, ref_pitch, cu_x + bx, cu_y + by, mx1, my1, patch[wave], mid[wave], lane, k);
    if (in_pic) {
      int v;
      if constexpr (WP == 2) {
        const MePredWp<1> a0 = wp.ref[0][i0], a1 = wp.ref[1][i1];
        if (use0 && use1) v = me_tail_weight_bi(sum0, sum1, a0.w0, a1.w0, (1 + a0.offset + a1.offset) * (1 << (wp.shift - 1)), wp.shift, k.maxv);
        else v = me_tail_weight_uni(use0 ? sum0 : sum1, use0 ? a0 : a1, k.maxv);   // wave-uniform
      } else if constexpr (WP == 1) {
        if (use0 && use1) v = me_tail_weight_bi(sum0, sum1, wp.w0, wp.w1, wp.add, wp.shift, k.maxv);
        else v = me_tail_weight_uni(use0 ? sum0 : sum1, use0 ? wp.uni[0] : wp.uni[1], k.maxv);   // wave-uniform
      } else {
        v = me_tail_dir(use0, use1, sum0, sum1, k);
      }
      me_store_sample<SrcT>(dst, dst_pitch, cu_x + bx + (lane & 7), cu_y + by + (lane >> 3), pic_w, pic_h, v);
    }
  }
}

// ---- L0, L1 or bi per 4x4 block (hmme_predict_bi4_device; the rule: include/hmme.h) -------------------------------------------------------
// me_predict_bi_kernel<SrcT> with HM's own motion storage: mv_field int16 [2][n_ctu][256][2] (list-major), dir_field uint8 [n_ctu][256], entry b
// the 4x4 block at ((b & 15) * 4, (b >> 4) * 4) of the CTU.  Lanes, patches and taps are me_predict4_kernel's; list 0 and then list 1 go
// through the same wave-private LDS (me_predict4_pass twice: FOUR barriers per iteration, as me_predict_bi_kernel has).  Direction and both
// MVs are per QUADRANT, read from the quadrant's first lane: a quadrant is live if its 4x4 block starts inside the picture and its direction
// is 1, 2 or 3; in a list its direction does not name it stages nothing.  Tail per lane: me_tail_avg when both lists are used, else
// me_tail_uni -- the sample me_predict_bi_kernel writes when the 8x8 block carries the quadrant's (direction, MV0, MV1).
// The barrier invariant is me_predict4_pass's: both passes of all 16 iterations are met by every wave, whatever the field holds.
//   REFS = 0: one reference per list, ref0 / ref1.  Takes an empty struct and compiles to what it did without the argument.
//   REFS = 1: a reference picture per 4x4 block and list (hmme_predict_bi_refs4_device): ref_field uint8 [2][n_ctu][256] (list-major, like the
//            MVs) names the plane of set[l] a block reads in list l (all of one pitch; ref0 / ref1 are not used).  The indices are per
//            QUADRANT like the direction, so the plane of a quadrant comes through readlane of a per-lane index, as in me_predict4_kernel.
//            A quadrant that uses a list whose index is >= n[l] (0xFF: no CU) is like one without a direction: it reads no plane and its
//            lanes write nothing.  The index of a list the quadrant does not use is not compared, and is clamped to 0 before any lookup.
//            Liveness still sits inside the stages only: the barrier invariant holds as it did.
template <typename SrcT, int REFS = 0>
__global__ void __launch_bounds__(256)
me_predict_bi4_kernel(const uint8_t* __restrict__ ref0, const uint8_t* __restrict__ ref1, int ref_pitch, const int16_t* __restrict__ mv_field,
                      const uint8_t* __restrict__ dir_field, int n_ctu, int ctu_first, int pic_w, int pic_h, int bit_depth, uint8_t* __restrict__ dst,
                      int dst_pitch, MePredBiRefs<REFS> refs) {
  __shared__ int16_t patch[4][4 * 11 * 12];
  __shared__ int16_t mid[4][4 * 11 * 4];
  __shared__ uint32_t taps[4][2];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  me_stage_luma_taps(taps);
  const auto [ctu, cx, cy, cu_x, cu_y] = me_pred_ctu(ctu_first, pic_w);
  const MePredConst k(bit_depth);
  const int r = lane >> 3, c = lane & 7;
#pragma unroll 1
  for (int it = 0; it < 16; ++it) {
    const int b = it * 4 + wave, bx = (b & 7) * 8, by = (b >> 3) * 8;   // the four waves: four 8x8 blocks side by side
    const int qx = bx + (c & 4), qy = by + (r & 4);                      // this lane's 4x4 block inside the CTU
    const long e = (long)ctu * 256 + (qy >> 2) * 16 + (qx >> 2);
    const int dir = dir_field[e];
    bool live = cu_x + qx < pic_w && cu_y + qy < pic_h && dir >= 1 && dir <= 3;
    [[maybe_unused]] int r0 = 0, r1 = 0;   // REFS: the lane's indices, 0 in a list it does not use
    if constexpr (REFS) {
      r0 = refs.ref_field[e]; r1 = refs.ref_field[(long)n_ctu * 256 + e];
      live = live && (!(dir & 1) || r0 < refs.n[0]) && (!(dir & 2) || r1 < refs.n[1]);
    }
    const bool use0 = live && (dir & 1), use1 = live && (dir & 2);
    int mx0 = 0, my0 = 0, mx1 = 0, my1 = 0;
    if (use0) me_field_mv(mv_field, e, cu_x, cu_y, pic_w, pic_h, mx0, my0);
    if (use1) me_field_mv(mv_field, (long)n_ctu * 256 + e, cu_x, cu_y, pic_w, pic_h, mx1, my1);
    int sum0, sum1;
    if constexpr (REFS) {
      if (!use0) r0 = 0;   // use0: r0 < n[0]
      if (!use1) r1 = 0;
      const auto plane0 = [&](int from) { return refs.set[0].base[__builtin_amdgcn_readlane(r0, from)]; };
      const auto plane1 = [&](int from) { return refs.set[1].base[__builtin_amdgcn_readlane(r1, from)]; };
      sum0 = me_predict4_pass<SrcT>(use0, plane0, ref_pitch, cu_x + bx, cu_y + by, mx0, my0, patch[wave], mid[wave], taps, lane, k);
      sum1 = me_predict4_pass<SrcT>(use1, plane1, ref_pitch, cu_x + bx, cu_y + by, mx1, my1, patch[wave], mid[wave], taps, lane, k);
    } else {
      sum0 = me_predict4_pass<SrcT>(use0, [=](int) { return ref0; }, ref_pitch, cu_x + bx, cu_y + by, mx0, my0, patch[wave], mid[wave], taps, lane, k);
      sum1 = me_predict4_pass<SrcT>(use1, [=](int) { return ref1; }, ref_pitch, cu_x + bx, cu_y + by, mx1, my1, patch[wave], mid[wave], taps, lane, k);
    }
    if (live) me_store_sample<SrcT>(dst, dst_pitch, cu_x + bx + c, cu_y + by + r, pic_w, pic_h, me_tail_dir(use0, use1, sum0, sum1, k));
  }
}

// ---- 4:2:0 chroma motion compensation from the luma motion fields (hmme_predict_chroma_*_device) -------------------------------------------
// TComPrediction::xPredInterBlk for a chroma component of a 4:2:0 picture (TComPrediction.cpp:669-707): the quarter-pel LUMA MV, clamped like
// clip_mv_q with the luma picture size and the CTU's luma position, is an eighth-pel chroma MV: integer offset mv >> 3 (arithmetic), phase
// mv & 7, four taps (m_chromaFilter, TComInterpolationFilter.cpp:65-75).  HM's three branches (horizontal only, vertical only, both through
// the 14-bit intermediate) are the ONE two-stage formula of me_predict_kernel with phase 0 as the filter {0, 64, 0, 0}.
// Taps by eighth-pel phase, one dword per phase (tap j = signed byte j): a lane fetches a block's four taps with one LDS read.
__constant__ uint32_t kChromaTaps[8] = {0x00004000u, 0xFE0A3AFEu, 0xFE1036FCu, 0xFC1C2EFAu, 0xFC2424FCu, 0xFA2E1CFCu, 0xFC3610FEu, 0xFE3A0AFEu};

// One list's two passes for a 16-lane GROUP: the 4x4 block of one component (one 8x8 luma block) at chroma position (x0, y0).  The 7 x 7
// patch -- rows / columns -1 .. +5 around the displaced block -- goes through LDS (patch: 7 rows of 8), the horizontal pass writes the 14-bit
// intermediate (mid: 7 rows of 4), and lane l16 = 4 r + c returns the vertical sum of sample (r, c) before any shift, so that the caller ends
// it with one of the tails.  origin, mx, my and live are the same for the 16 lanes of a group (and for the 32 of a
// luma block's two components, apart from origin); a group that is not live reads nothing and still meets both barriers.
template <typename SrcT>
__device__ __forceinline__ int me_predict_chroma_sum(bool live, const uint8_t* origin, int ref_pitch, int x0, int y0, int mx, int my, int16_t* patch,
                                                     int16_t* mid, int l16, const uint32_t* taps, const MePredConst& k) {
  if (live) {
    const uint8_t* src = origin + (long)(y0 + (my >> 3) - 1) * ref_pitch + (long)(x0 + (mx >> 3) - 1) * (long)sizeof(SrcT);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = l16 + 16 * j, r = e / 7, c = e - r * 7;
      if (e < 49) patch[r * 8 + c] = (int16_t)((const SrcT*)(src + (long)r * ref_pitch))[c];
    }
  }
  __syncthreads();
  if (live) {
    const uint32_t th = taps[mx & 7];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int o = l16 + 16 * j, r = o >> 2, c = o & 3;
      if (o < 28) {
        int sum = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) sum += (int)(int8_t)(th >> (8 * t)) * (int)patch[r * 8 + c + t];
        mid[o] = (int16_t)((sum + k.off1) >> k.sh1);
      }
    }
  }
  __syncthreads();
  int sum = 0;
  if (live) {
    const uint32_t tv = taps[my & 7];
    const int r = l16 >> 2, c = l16 & 3;
#pragma unroll
    for (int t = 0; t < 4; ++t) sum += (int)(int8_t)(tv >> (8 * t)) * (int)mid[(r + t) * 4 + c];
  }
  return sum;
}

// The three forms of the luma prediction for Cb and Cr in ONE launch: one LUMA CTU (a 32 x 32 chroma area per component) per workgroup.
// A wave carries two 8x8 luma blocks x two components, a lane one output sample: lane = 32 * (block of the pair) + 16 * component +
// 4 * row + column, the four waves take the eight blocks of one block row, eight iterations per CTU.  MV, phase, direction and
// reference index are uniform per 32 lanes, the plane per 16.  PER = mv_per_ctu (1 | 64): with 1 they are the same for the whole workgroup
// and stay in scalar registers.  Planes and weights come in component pairs (entry 2 i: Cb, 2 i + 1: Cr of picture / reference i), all
// planes of one pitch; pic_w / pic_h are the LUMA size (even), the fields are indexed by luma CTUs.
//   FORM 0: me_predict_kernel<SrcT, 0, WP>: one plane pair (hmme_predict_chroma_pairs_device); WP = 1: one MePredWp<1> per component
//   FORM 1: me_predict_kernel<SrcT, 0, WP, 1>: ref_field uint8 [n_ctu][PER] names the plane pair of `set` (hmme_predict_chroma_refs_device);
//           WP = 2: the MePredWp<1> of plane 2 * index + component.  An index >= n_refs is not live.
//   FORM 2: me_predict_bi_kernel<SrcT, WP>: mv_field int16 [2][n_ctu][PER][2], dir_field uint8 [n_ctu][PER], set.base[0..1] list 0, [2..3]
//           list 1 (hmme_predict_chroma_bi_device); WP = 1: one MePredBiWp<1> per component.  A direction outside 1..3 is not live.
//   FORM 3: me_predict_bi_kernel<SrcT, WP, 1>: FORM 2 with a reference per block and list (hmme_predict_chroma_bi_refs_device): wp.ref_field
//           uint8 [2][n_ctu][PER] is read beside the direction; set.base[2 * r + comp] is list 0's reference r (r < n_refs), set.base[2 *
//           (n_refs + r) + comp] list 1's (r < n_refs1).  A block that uses a list whose index is beyond it is not live.  WP = 2: the
//           MePredWp<1> of every plane, indexed like set.base -- the indices are uniform per 32 lanes, not per wave, so this is a per-lane
//           index; the weights are therefore staged into LDS beside the taps, which keeps the kernel arguments out of scratch.  An index
//           that is not used is clamped to 0 before any lookup.
// The tails are the luma kernels' (WP = 0: me_tail_uni / me_tail_avg; else me_tail_weight_uni / me_tail_weight_bi), with the component's own
// weight.  A block that is not live -- or whose luma block lies wholly outside
// the picture -- reads no plane and writes nothing, and still meets every barrier.  Stores are samples of the planes' type, only inside the
// chroma picture.
struct MeChromaSrc { RefSet set; const uint8_t* field; int n_refs, n_ctu; };   // field: ref_field (FORM 1) / dir_field (FORM 2, 3)
template <int FORM, int WP> struct MeChromaWp {};
template <> struct MeChromaWp<0, 1> { MePredWp<1> c[2]; };
template <> struct MeChromaWp<1, 2> { MePredWp<1> ref[kMaxRefs]; };
template <> struct MeChromaWp<2, 1> { MePredBiWp<1> c[2]; };
// FORM 3 carries its second field and list 1's count here, so that MeChromaSrc stays what the other forms take
template <> struct MeChromaWp<3, 0> { const uint8_t* ref_field; int n_refs1; };
template <> struct MeChromaWp<3, 2> { const uint8_t* ref_field; int n_refs1; int shift[2]; MePredWp<1> ref[kMaxRefs]; };   // ref[plane], indexed like set.base; shift[comp]: the bi shift'
template <typename SrcT, int FORM, int WP, int PER>
__global__ void __launch_bounds__(256)
me_predict_chroma_kernel(MeChromaSrc src, int ref_pitch, const int16_t* __restrict__ mv_field, int ctu_first, int pic_w, int pic_h, int bit_depth,
                         uint8_t* __restrict__ dst_cb, uint8_t* __restrict__ dst_cr, int dst_pitch, MeChromaWp<FORM, WP> wp) {
  __shared__ int16_t patch[16][7 * 8];
  __shared__ int16_t mid[16][7 * 4];
  __shared__ uint32_t taps[8];
  const int group = threadIdx.x >> 4, l16 = threadIdx.x & 15, comp = group & 1;
  if (threadIdx.x < 8) taps[threadIdx.x] = kChromaTaps[threadIdx.x];   // read behind the first barrier of the first pass
  const int* s_wp = nullptr;   // FORM 3, WP 2: the planes' weights in LDS, read behind the barriers, too
  if constexpr (FORM == 3 && WP == 2) {
    __shared__ int s_weights[kMaxRefs * 4];
    me_stage_weights(s_weights, wp.ref);
    s_wp = s_weights;
  }
  const auto [ctu, cx, cy, cu_x, cu_y] = me_pred_ctu(ctu_first, pic_w);
  const MePredConst k(bit_depth);
  uint8_t* const dst = comp ? dst_cr : dst_cb;
#pragma unroll 1
  for (int it = 0; it < 8; ++it) {
    const int b = it * 8 + (group >> 1), bx = (b & 7) * 8, by = it * 8;   // luma block of the CTU: a block row per iteration
    const long e = (long)ctu * PER + (PER == 1 ? 0 : b);
    const bool in_pic = cu_x + bx < pic_w && cu_y + by < pic_h;
    const int x0 = (cu_x + bx) >> 1, y0 = (cu_y + by) >> 1;
    bool use0 = in_pic, use1 = false;
    int sel = 0;   // FORM 1: the reference index
    if constexpr (FORM == 1) {
      sel = src.field[e];
      use0 = use0 && sel < src.n_refs;
      if (!use0) sel = 0;
    }
    if constexpr (FORM == 2) {
      const int dir = src.field[e];
      const bool ok = in_pic && dir >= 1 && dir <= 3;
      use0 = ok && (dir & 1); use1 = ok && (dir & 2);
    }
    int sel1 = 1;   // the plane pair of list 1: FORM 2's second pair, FORM 3: n_refs + the index
    if constexpr (FORM == 3) {
      const int dir = src.field[e], r0 = wp.ref_field[e], r1 = wp.ref_field[(long)src.n_ctu * PER + e];
      const bool ok = in_pic && dir >= 1 && dir <= 3 && (!(dir & 1) || r0 < src.n_refs) && (!(dir & 2) || r1 < wp.n_refs1);
      use0 = ok && (dir & 1); use1 = ok && (dir & 2);
      sel = use0 ? r0 : 0;
      sel1 = src.n_refs + (use1 ? r1 : 0);
    }
    int mx0 = 0, my0 = 0, mx1 = 0, my1 = 0;
    if (use0) me_field_mv(mv_field, e, cu_x, cu_y, pic_w, pic_h, mx0, my0);
    const int sum0 = me_predict_chroma_sum<SrcT>(use0, src.set.base[2 * sel + comp], ref_pitch, x0, y0, mx0, my0, patch[group], mid[group], l16, taps, k);
    int sum1 = 0;
    if constexpr (FORM >= 2) {
      if (use1) me_field_mv(mv_field, (long)src.n_ctu * PER + e, cu_x, cu_y, pic_w, pic_h, mx1, my1);
      sum1 = me_predict_chroma_sum<SrcT>(use1, src.set.base[2 * sel1 + comp], ref_pitch, x0, y0, mx1, my1, patch[group], mid[group], l16, taps, k);
    }
    if (use0 || use1) {
      int v;
      if constexpr (WP == 0) {
        v = me_tail_dir(use0, use1, sum0, sum1, k);
      } else if (FORM >= 2 && use0 && use1) {
        if constexpr (FORM == 2) v = me_tail_weight_bi(sum0, sum1, wp.c[comp].w0, wp.c[comp].w1, wp.c[comp].add, wp.c[comp].shift, k.maxv);
        else if constexpr (FORM == 3) {
          const MePredWp<1> a0 = me_staged_weight(s_wp, 2 * sel + comp), a1 = me_staged_weight(s_wp, 2 * sel1 + comp);
          const int sh = wp.shift[comp];
          v = me_tail_weight_bi(sum0, sum1, a0.w0, a1.w0, (1 + a0.offset + a1.offset) * (1 << (sh - 1)), sh, k.maxv);
        }
      } else {
        MePredWp<1> w;
        if constexpr (FORM == 0) w = wp.c[comp];
        else if constexpr (FORM == 1) w = wp.ref[2 * sel + comp];
        else if constexpr (FORM == 3) w = me_staged_weight(s_wp, 2 * (use0 ? sel : sel1) + comp);
        else w = wp.c[comp].uni[use0 ? 0 : 1];
        v = me_tail_weight_uni(use0 ? sum0 : sum1, w, k.maxv);
      }
      me_store_sample<SrcT>(dst, dst_pitch, x0 + (l16 & 3), y0 + (l16 >> 2), pic_w >> 1, pic_h >> 1, v);
    }
  }
}

// me_predict_chroma4_pass is one list's pass for a 16-lane group -- the 4x4 block of one component at chroma position (x0, y0) -- and the only
// place that stages, filters and sums quads (me_predict_chroma4_kernel: one pass per iteration; me_predict_chroma_bi4_kernel: list 0's, then
// list 1's).  live, mx, my are the LANE's -- those of its quad; plane_of(from) is the plane of the quad whose first lane is `from`, called
// by the whole wave for every quad, live or not (a quad that is not live reads nothing from it).  Returns the vertical sum of lane (r, c) before any shift (0 in a lane that is not live).
//   stage       per quad the 5 x 5 patch at its MV -- rows / columns -1 .. +3 around the displaced 2x2 block, a subset of the 7 x 7 patch of
//               the 64 form at that MV -- into the group's LDS, quad by quad; a quad's entry comes from its first lane (__shfl)
//   horizontal  5 rows x 2 columns per quad, 40 outputs per group in three steps, taps by the output's quad
//   vertical    lane (r, c): four rows of its quad's intermediate
// Two barriers, both outside every branch: the BARRIER INVARIANT is stated at me_predict4_pass and holds here word for word.
template <typename SrcT, class PlaneOf>
__device__ __forceinline__ int me_predict_chroma4_pass(bool live, PlaneOf plane_of, int ref_pitch, int x0, int y0, int mx, int my, int16_t* gpatch,
                                                       int16_t* gmid, const uint32_t* taps, int lane, const MePredConst& k) {
  const int l16 = lane & 15, r = l16 >> 2, c = l16 & 3, q = (r >> 1) * 2 + (c >> 1);
  int info[4];   // per group: 8 | horizontal phase of a live quad, else 0
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int from = (lane & 48) + (s >> 1) * 8 + (s & 1) * 2;
    const int s_live = __shfl((int)live, from), s_mx = __shfl(mx, from), s_my = __shfl(my, from);
    const uint8_t* const plane = plane_of(from);   // in front of the branch: a cross-lane read in it goes out with the three above
    info[s] = s_live ? 8 | (s_mx & 7) : 0;
    if (s_live) {
      const uint8_t* p = plane + (long)(y0 + (s >> 1) * 2 + (s_my >> 3) - 1) * ref_pitch + (long)(x0 + (s & 1) * 2 + (s_mx >> 3) - 1) * (long)sizeof(SrcT);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int el = l16 + 16 * j, pr = el / 5, pc = el - pr * 5;
        if (el < 25) gpatch[s * 25 + el] = (int16_t)((const SrcT*)(p + (long)pr * ref_pitch))[pc];
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int o = l16 + 16 * j, oq = o / 10, rem = o - oq * 10;   // output (row rem >> 1, column rem & 1) of quad oq
    const int inf = oq == 0 ? info[0] : (oq == 1 ? info[1] : (oq == 2 ? info[2] : info[3]));
    if (o < 40 && inf) {
      const uint32_t th = taps[inf & 7];
      const int16_t* p = gpatch + oq * 25 + (rem >> 1) * 5 + (rem & 1);
      int sum = 0;
#pragma unroll
      for (int t = 0; t < 4; ++t) sum += (int)(int8_t)(th >> (8 * t)) * (int)p[t];
      gmid[o] = (int16_t)((sum + k.off1) >> k.sh1);
    }
  }
  __syncthreads();
  int sum = 0;
  if (live) {
    const uint32_t tv = taps[my & 7];
    const int16_t* p = gmid + q * 10 + (r & 1) * 2 + (c & 1);
#pragma unroll
    for (int t = 0; t < 4; ++t) sum += (int)(int8_t)(tv >> (8 * t)) * (int)p[2 * t];
  }
  return sum;
}

// FORM 1 from one MV per 4x4 LUMA block (hmme_predict_chroma_refs4_device): mv_field int16 [n_ctu][256][2], src.field uint8 [n_ctu][256]
// (null: every block index 0).  The lanes are those of me_predict_chroma_kernel -- a 16-lane group owns the 4x4 block of one component of
// one 8x8 luma block, lane l16 = 4 r + c one sample, eight iterations per CTU -- but the block is four 2x2 QUADS, lane (r, c) in quad
// (r >> 1) * 2 + (c >> 1), each the chroma of one 4x4 luma block with that block's MV (the CTU's clamp), reference index and the
// component's weight of that reference: sample for sample what the 64 form writes when the 8x8 luma block carries the entry.
// One me_predict_chroma4_pass per iteration, the plane of a quad being set.base[2 * its index + component]; then me_tail_uni (WP = 0) or
// me_tail_weight_uni with the weight of that plane (WP = 2; me_stage_weights, because the index is per lane).
// A quad is live if its 4x4 luma block starts inside the luma picture and its index is < n_refs.  The barrier invariant is the pass's: the
// loop has eight iterations for every group of every wave.
template <typename SrcT, int WP>
__global__ void __launch_bounds__(256)
me_predict_chroma4_kernel(MeChromaSrc src, int ref_pitch, const int16_t* __restrict__ mv_field, int ctu_first, int pic_w, int pic_h, int bit_depth,
                          uint8_t* __restrict__ dst_cb, uint8_t* __restrict__ dst_cr, int dst_pitch, MeChromaWp<1, WP> wp) {
  static_assert(WP == 0 || WP == 2, "one weight per plane, or none");
  __shared__ int16_t patch[16][4 * 25];
  __shared__ int16_t mid[16][4 * 10];
  __shared__ uint32_t taps[8];
  __shared__ int s_weights[kMaxRefs * 4];
  const int group = threadIdx.x >> 4, l16 = threadIdx.x & 15, comp = group & 1, lane = threadIdx.x & 63;
  if (threadIdx.x < 8) taps[threadIdx.x] = kChromaTaps[threadIdx.x];   // read behind the first barrier
  if constexpr (WP == 2) me_stage_weights(s_weights, wp.ref);
  const auto [ctu, cx, cy, cu_x, cu_y] = me_pred_ctu(ctu_first, pic_w);
  const MePredConst k(bit_depth);
  uint8_t* const dst = comp ? dst_cr : dst_cb;
  const int r = l16 >> 2, c = l16 & 3;
#pragma unroll 1
  for (int it = 0; it < 8; ++it) {
    const int bx = (group >> 1) * 8, by = it * 8;                        // the group's 8x8 luma block: a block row per iteration
    const int qx = bx + (c >> 1) * 4, qy = by + (r >> 1) * 4;           // this lane's 4x4 luma block inside the CTU
    const long e = (long)ctu * 256 + (qy >> 2) * 16 + (qx >> 2);
    const int x0 = (cu_x + bx) >> 1, y0 = (cu_y + by) >> 1;
    int sel = src.field ? (int)src.field[e] : 0;
    const bool live = cu_x + qx < pic_w && cu_y + qy < pic_h && sel < src.n_refs;
    int mx = 0, my = 0;
    if (live) me_field_mv(mv_field, e, cu_x, cu_y, pic_w, pic_h, mx, my);
    else sel = 0;
    const auto plane_of = [&](int from) { return src.set.base[2 * __shfl(sel, from) + comp]; };
    const int sum = me_predict_chroma4_pass<SrcT>(live, plane_of, ref_pitch, x0, y0, mx, my, patch[group], mid[group], taps, lane, k);
    if (live) {
      int v;
      if constexpr (WP == 2) v = me_tail_weight_uni(sum, me_staged_weight(s_weights, 2 * sel + comp), k.maxv);
      else v = me_tail_uni(sum, k);
      me_store_sample<SrcT>(dst, dst_pitch, x0 + c, y0 + r, pic_w >> 1, pic_h >> 1, v);
    }
  }
}

// me_predict_chroma4_kernel's sibling for a direction per 4x4 luma block (hmme_predict_chroma_bi4_device): FORM 2 of me_predict_chroma_kernel
// from the 256 layout, unweighted.  mv_field int16 [2][n_ctu][256][2], src.field = dir_field uint8 [n_ctu][256], src.set.base[0..1] list 0's
// Cb / Cr, [2..3] list 1's.  Groups, lanes, quads and patches are me_predict_chroma4_kernel's; list 0 and then list 1 go through the group's
// LDS (me_predict_chroma4_pass twice: FOUR barriers per iteration).  A quad is live if its 4x4 luma block starts inside the luma picture and
// its direction is 1, 2 or 3.  Tail per lane: me_tail_avg when both lists are used, else me_tail_uni.
// The barrier invariant is the pass's: both passes of all eight iterations are met by every group of every wave, whatever the field holds.
//   REFS = 0: one reference per list (MeChromaWp<2, 0>: empty).  Compiles to what it did without the argument.
//   REFS = 1: FORM 3 from the 256 layout, unweighted (hmme_predict_chroma_bi_refs4_device): refs.ref_field uint8 [2][n_ctu][256] is read
//            beside the direction; set.base[2 * r + comp] is list 0's reference r (r < src.n_refs), set.base[2 * (src.n_refs + r) + comp]
//            list 1's (r < refs.n_refs1).  The plane of a quad comes from its first lane's index (__shfl), as in me_predict_chroma4_kernel.
//            A quad that uses a list whose index is beyond it is not live; an index that is not used is clamped to 0 before any lookup.
template <typename SrcT, int REFS = 0>
__global__ void __launch_bounds__(256)
me_predict_chroma_bi4_kernel(MeChromaSrc src, int ref_pitch, const int16_t* __restrict__ mv_field, int ctu_first, int pic_w, int pic_h, int bit_depth,
                             uint8_t* __restrict__ dst_cb, uint8_t* __restrict__ dst_cr, int dst_pitch, MeChromaWp<REFS ? 3 : 2, 0> refs) {
  __shared__ int16_t patch[16][4 * 25];
  __shared__ int16_t mid[16][4 * 10];
  __shared__ uint32_t taps[8];
  const int group = threadIdx.x >> 4, l16 = threadIdx.x & 15, comp = group & 1, lane = threadIdx.x & 63;
  if (threadIdx.x < 8) taps[threadIdx.x] = kChromaTaps[threadIdx.x];   // read behind the first barrier
  const auto [ctu, cx, cy, cu_x, cu_y] = me_pred_ctu(ctu_first, pic_w);
  const MePredConst k(bit_depth);
  uint8_t* const dst = comp ? dst_cr : dst_cb;
  const uint8_t* const plane0 = src.set.base[comp];
  const uint8_t* const plane1 = src.set.base[2 + comp];
  const int r = l16 >> 2, c = l16 & 3;
#pragma unroll 1
  for (int it = 0; it < 8; ++it) {
    const int bx = (group >> 1) * 8, by = it * 8;                        // the group's 8x8 luma block: a block row per iteration
    const int qx = bx + (c >> 1) * 4, qy = by + (r >> 1) * 4;           // this lane's 4x4 luma block inside the CTU
    const long e = (long)ctu * 256 + (qy >> 2) * 16 + (qx >> 2);
    const int x0 = (cu_x + bx) >> 1, y0 = (cu_y + by) >> 1;
    const int dir = src.field[e];
    bool live = cu_x + qx < pic_w && cu_y + qy < pic_h && dir >= 1 && dir <= 3;
    [[maybe_unused]] int r0 = 0, r1 = 0;   // REFS: the lane's indices, 0 in a list it does not use
    if constexpr (REFS) {
      r0 = refs.ref_field[e]; r1 = refs.ref_field[(long)src.n_ctu * 256 + e];
      live = live && (!(dir & 1) || r0 < src.n_refs) && (!(dir & 2) || r1 < refs.n_refs1);
    }
    const bool use0 = live && (dir & 1), use1 = live && (dir & 2);
    int mx0 = 0, my0 = 0, mx1 = 0, my1 = 0;
    if (use0) me_field_mv(mv_field, e, cu_x, cu_y, pic_w, pic_h, mx0, my0);
    if (use1) me_field_mv(mv_field, (long)src.n_ctu * 256 + e, cu_x, cu_y, pic_w, pic_h, mx1, my1);
    int sum0, sum1;
    if constexpr (REFS) {
      if (!use0) r0 = 0;   // use0: r0 < n_refs
      if (!use1) r1 = 0;
      const auto of0 = [&](int from) { return src.set.base[2 * __shfl(r0, from) + comp]; };
      const auto of1 = [&](int from) { return src.set.base[2 * (src.n_refs + __shfl(r1, from)) + comp]; };
      sum0 = me_predict_chroma4_pass<SrcT>(use0, of0, ref_pitch, x0, y0, mx0, my0, patch[group], mid[group], taps, lane, k);
      sum1 = me_predict_chroma4_pass<SrcT>(use1, of1, ref_pitch, x0, y0, mx1, my1, patch[group], mid[group], taps, lane, k);
    } else {
      sum0 = me_predict_chroma4_pass<SrcT>(use0, [=](int) { return plane0; }, ref_pitch, x0, y0, mx0, my0, patch[group], mid[group], taps, lane, k);
      sum1 = me_predict_chroma4_pass<SrcT>(use1, [=](int) { return plane1; }, ref_pitch, x0, y0, mx1, my1, patch[group], mid[group], taps, lane, k);
    }
    if (live) me_store_sample<SrcT>(dst, dst_pitch, x0 + c, y0 + r, pic_w >> 1, pic_h >> 1, me_tail_dir(use0, use1, sum0, sum1, k));
  }
}

// ---- estimating explicit weighted-prediction parameters (hmme_plane_stats / hmme_wp_estimate / hmme_wp_estimate_420) -------------------------
// The whole-picture reductions of HM's WeightPredAnalysis (WeightPredAnalysis.cpp:67-120 xCalcACDCParamSlice, :324-351 xCalcSADvalueWP) over
// the PICTURE AREA of padded planes -- no margin, no replicated edge -- for SEVERAL planes of different sizes in one launch: blockIdx.y names
// a plane (statistics) or a pair of planes (SAD) of a table passed by value, like RefSet.  A luma call is a set of one plane, of 1 + n planes or
// of n pairs; a 4:2:0 call with 16 references has 51 planes and 48 pairs.
// Geometry shared by both kernels: a workgroup of 256 lanes is (256 >> lpr_log2) rows of (1 << lpr_log2) lanes, lpr = the smallest power of two
// that covers a row's 16-byte vectors (at most 256), so narrow pictures keep their lanes busy and nothing is divided; rows advance by
// gridDim.x * rows-per-workgroup, a row's vectors by lpr.  Every plane brings its own lpr_log2, so rows per workgroup differ between the
// planes of a launch.  The picture's left edge is 128 samples into a pitch that is a multiple of 256 bytes, so every vector is a 16-byte
// aligned load; the last vector of a row may reach into the right margin (128 samples: always inside the row) and is masked to the row's bytes.
// gridDim.x is sized for the plane that needs most workgroups; a workgroup whose first row lies beyond its (smaller) plane has nothing to add
// and LEAVES AS A WHOLE, before any barrier (the one of the pass-1 mean, those of me_block_sum_u64): the test is on blockIdx and the plane's
// table entry only, the same for all 256 lanes.  The sums are zero on entry, so a sum nobody adds to is the right one.
// Sums: one 32-bit partial per vector (bounds at the kernels), widened into a 64-bit lane sum right away; lanes are folded wave by wave with a
// butterfly, the four wave sums through LDS, and ONE 64-bit atomic add per workgroup and sum reaches memory.  Integer adds only: the result
// does not depend on the order of workgroups, nor on the grid.

// the bytes of dword k that belong to a row of which nb (1..15) bytes lie in the vector
__device__ __forceinline__ uint32_t me_tail_mask(int nb, int k) {
  const int vb = nb - 4 * k;
  return vb >= 4 ? 0xffffffffu : vb <= 0 ? 0u : (1u << (8 * vb)) - 1u;
}
// packed sum of absolute differences of one dword of samples + acc: v_sad_u8 (four u8) / v_sad_u16 (two u16)
template <typename T>
__device__ __forceinline__ uint32_t me_sad_packed(uint32_t a, uint32_t b, uint32_t acc) {
  if (sizeof(T) == 1) return __builtin_amdgcn_sad_u8(a, b, acc);
  return __builtin_amdgcn_sad_u16(a, b, acc);
}
template <int NSUM>
__device__ __forceinline__ void me_block_sum_u64(uint64_t (&v)[NSUM], unsigned long long* out) {
  __shared__ uint64_t s_part[4][NSUM];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < NSUM; ++k) {
#pragma unroll
    for (int mask = 32; mask >= 1; mask >>= 1) v[k] += me_shfl_xor_u64(v[k], mask);
    if (lane == 0) s_part[wave][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < NSUM)
    atomicAdd(out + threadIdx.x, (unsigned long long)(s_part[0][threadIdx.x] + s_part[1][threadIdx.x] + s_part[2][threadIdx.x] + s_part[3][threadIdx.x]));
}

constexpr int kMaxSetPlanes = 3 * (kMaxRefs + 1);   // Y, Cb, Cr of the current picture and of kMaxRefs references
constexpr int kMaxSetPairs = 3 * kMaxRefs;
struct MePlaneDesc { const uint8_t* origin; int pitch, w, h, lpr_log2; };
struct MePlaneSet { MePlaneDesc p[kMaxSetPlanes]; };

// xCalcACDCParamSlice of one plane of a launch in two launches on one stream, sums[0] / sums[1] = its sample sum / AC.  PASS 0: sums[0] += sum
// of the samples (iOrgDC; v_sad against 0).  PASS 1: reads the plane's sum as pass 0 left it, normDC = (iOrgDC + (N >> 1)) / N (:99),
// sums[1] += sum of |sample - normDC| (iOrgAC; v_sad against the replicated mean).  All planes of a launch hold samples of type T (one bit
// depth per call).  A vector's partial is at most 16 * 255 / 8 * 4095.
template <typename T, int PASS>
__device__ __forceinline__ void me_plane_stats_body(const MePlaneDesc& pd, unsigned long long* sums) {
  __shared__ uint32_t s_mean;
  const int lpr = 1 << pd.lpr_log2, lx = threadIdx.x & (lpr - 1), ry = threadIdx.x >> pd.lpr_log2, rpb = 256 >> pd.lpr_log2;
  if ((int)blockIdx.x * rpb >= pd.h) return;   // the whole workgroup: no lane has a row
  uint32_t mean = 0;   // the mean in every sample of a dword
  if (PASS == 1) {
    if (threadIdx.x == 0) {
      const unsigned long long n = (unsigned long long)pd.w * (unsigned long long)pd.h;
      s_mean = (uint32_t)((sums[0] + (n >> 1)) / n);
    }
    __syncthreads();
    mean = s_mean * (sizeof(T) == 1 ? 0x01010101u : 0x00010001u);
  }
  const int row_bytes = pd.w * (int)sizeof(T), nvec = (row_bytes + 15) >> 4;
  uint64_t acc[1] = {0};
  for (int y = blockIdx.x * rpb + ry; y < pd.h; y += gridDim.x * rpb) {
    const uint8_t* row = pd.origin + (long)y * pd.pitch;
    for (int v = lx; v < nvec; v += lpr) {
      const uint4 in = *(const uint4*)(row + 16 * v);
      const uint32_t d[4] = {in.x, in.y, in.z, in.w};
      const int nb = row_bytes - 16 * v;
      uint32_t part = 0;
      if (nb >= 16) {
#pragma unroll
        for (int k = 0; k < 4; ++k) part = me_sad_packed<T>(d[k], mean, part);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint32_t m = me_tail_mask(nb, k);
          part = me_sad_packed<T>(d[k] & m, mean & m, part);
        }
      }
      acc[0] += part;
    }
  }
  me_block_sum_u64<1>(acc, sums + PASS);
}
// plane p = blockIdx.y of the table: sums[2 p] / sums[2 p + 1]
template <typename T, int PASS>
__global__ void __launch_bounds__(256)
me_plane_set_stats_kernel(MePlaneSet set, unsigned long long* sums) {
  me_plane_stats_body<T, PASS>(set.p[blockIdx.y], sums + 2 * blockIdx.y);
}
// a set of ONE plane without the table: the 1.2 KB argument costs a launch of a single 2160p plane 0.25 us of its 11.5
template <typename T, int PASS>
__global__ void __launch_bounds__(256)
me_plane_stats_kernel(MePlaneDesc pd, unsigned long long* sums) {
  me_plane_stats_body<T, PASS>(pd, sums);
}

// xCalcSADvalueWP for up to kMaxSetPairs pairs (current plane, reference plane) in one launch: pair y = comps * reference + component reads
// component y % comps of the current picture -- comps = 1 (a luma call: every pair against cur[0]) or 3 -- whose size, pitch and lpr_log2 are
// the pair's (a reference plane has its component's size and so its pitch), with the pair's own (weight, offset, log2Denom); offset arrives as
// HM's term iOffset << (log2Denom + bitDepth - 8).  comps is a kernel argument and y is blockIdx.y: the plane is the same for all 256 lanes.
// Per pair two sums:
//   sums[2 y]     += sum of |(org << d) - (ref * weight + offset)|      (:344; int32 multiply-add)
//   sums[2 y + 1] += sum of |org - ref|                                 (packed SAD; HM's unweighted sum is this << d exactly)
// so one read of the two planes serves both of HM's calls.  Bounds: the estimator hands over weight in [0, 1920] (dWeight clipped to 15,
// d <= 7) and an offset, luma's or chroma's, that ends in Clip3(-128, 127) (WeightPredAnalysis.cpp:244, :248), so |offset term| <= 128 << 11 =
// 2^18 at d <= 7; a 12-bit sample's term is below 4095 * 1920 + 2^19 + 2^18 < 2^23 and a vector's partial (8 of them; 16 at 8 bit, each below
// 2^19) below 2^26 -- far inside 32 bits; the lane sums are 64-bit.
struct MeWpSadSet {
  int comps;
  MePlaneDesc cur[3];
  const uint8_t* ref[kMaxSetPairs];
  int weight[kMaxSetPairs], offset[kMaxSetPairs], log2_denom[kMaxSetPairs];
};

template <typename T>
__global__ void __launch_bounds__(256)
me_wp_sad_set_kernel(MeWpSadSet a, unsigned long long* sums) {
  constexpr int PER = 4 / (int)sizeof(T);   // samples per dword
  const int pair = blockIdx.y;
  const MePlaneDesc pd = a.cur[a.comps == 1 ? 0 : pair % 3];
  const int lpr = 1 << pd.lpr_log2, lx = threadIdx.x & (lpr - 1), ry = threadIdx.x >> pd.lpr_log2, rpb = 256 >> pd.lpr_log2;
  if ((int)blockIdx.x * rpb >= pd.h) return;   // the whole workgroup: no lane has a row
  const uint8_t* __restrict__ cur = pd.origin;
  const uint8_t* __restrict__ ref = a.ref[pair];
  const int wt = a.weight[pair], off = a.offset[pair], d = a.log2_denom[pair];
  const int row_bytes = pd.w * (int)sizeof(T), nvec = (row_bytes + 15) >> 4;
  uint64_t acc[2] = {0, 0};
  auto sample = [](uint32_t dw, int j) -> int { return sizeof(T) == 1 ? (int)((dw >> (8 * j)) & 0xffu) : (int)((dw >> (16 * j)) & 0xffffu); };
  for (int y = blockIdx.x * rpb + ry; y < pd.h; y += gridDim.x * rpb) {
    const long row = (long)y * pd.pitch;
    for (int v = lx; v < nvec; v += lpr) {
      const uint4 o4 = *(const uint4*)(cur + row + 16 * v), r4 = *(const uint4*)(ref + row + 16 * v);
      const uint32_t o[4] = {o4.x, o4.y, o4.z, o4.w}, q[4] = {r4.x, r4.y, r4.z, r4.w};
      const int nb = row_bytes - 16 * v;
      uint32_t pw = 0, pn = 0;
      if (nb >= 16) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          pn = me_sad_packed<T>(o[k], q[k], pn);
#pragma unroll
          for (int j = 0; j < PER; ++j) {
            const int t = (sample(o[k], j) << d) - (sample(q[k], j) * wt + off);
            pw += (uint32_t)(t < 0 ? -t : t);
          }
        }
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint32_t m = me_tail_mask(nb, k);
          pn = me_sad_packed<T>(o[k] & m, q[k] & m, pn);
#pragma unroll
          for (int j = 0; j < PER; ++j) {
            const int t = (sample(o[k], j) << d) - (sample(q[k], j) * wt + off);
            if ((4 * k + j * (int)sizeof(T)) < nb) pw += (uint32_t)(t < 0 ? -t : t);
          }
        }
      }
      acc[0] += pw;
      acc[1] += pn;
    }
  }
  me_block_sum_u64<2>(acc, sums + 2 * pair);
}

}  // namespace hmme
