// Fused TransformerModel/ICU local training, on-chip edition (reference training loop client.py:75-111,
// model src/Model.py:166-246).  ONE persistent launch trains every client of a rank for all its local
// epochs; each client runs on four co-resident 512-thread workgroups (head half H0 | head half H1 | vitals branch |
// labs branch): the branches and the head hand activations and gradients to each other once per direction per step,
// and the head halves exchange their rows once per step off the critical path (head_main).
//
// What differs from transformer.hip: after the prologue NOTHING of a client's model lives in global
// memory.  Per workgroup:
//   * the head's fp32 master weights and the branches' compact entries (biases, LayerNorm, the small dense /
//     ffn weights) stay in REGISTERS for the whole round (one class, no AGPRs: onchip.h ar / aw); their Adam
//     moments, and the branches' 64 x 64 v / out_proj blocks (weights AND moments), sit in a per-workgroup
//     workspace slab that each update phase loads ahead of its arithmetic (L2-resident; see br_update for why the
//     blocks moved there);
//   * bf16 weight images (the MFMA operands) and an fp32 copy of the bias / LayerNorm vectors live in
//     LDS; Adam rewrites them in place;
//   * activations chain in registers: every GEMM is computed transposed, Y^T = W . X^T, so the
//     16x16x32 MFMA leaves lane (b, g) of wave w holding features 16t + 4g + i of batch row 16w + b
//     ("T layout") — exactly the B operand of the next GEMM once the weight image's K axis is stored in
//     the matching permuted order (pcol below).  The forward and the d(input) backward of a wave never
//     leave its registers and need no barrier; LayerNorm row sums are in-lane + two permlane swaps;
//   * the activations the weight gradients need (X and dY of every dW = dY^T X) are written to
//     XOR-swizzled LDS tiles as they are produced and read back with ds_read_b64_tr_b16; each wave starts
//     the weight-gradient work its inputs allow as soon as its own backward is done, tracked by LDS progress
//     counters instead of a barrier (br_update), so the waves that finish the backward first work while the
//     rest are still in theirs;
//   * the only global traffic in the step loop is the next batch's input rows (prefetched during the
//     hand-off wait) and the hand-offs themselves: per wave 2 KB of bf16 rows as {value, step tag}
//     granules in 16-byte write-through (sc1) stores, swept with sc1 loads until every tag matches — the
//     data is the flag (cdna_hip_programming.md Guideline 16 R2): no drain on the producer, one round trip
//     on the consumer.
// Numerics are those of transformer.hip: bf16 MFMA operands with fp32 accumulation, fp32 elementwise
// math, exact-erf GELU, hash dropout masks (tf_common.h), torch.optim.Adam with a fresh state per round.
#include "common.h"
#include "kernels.h"
#include "tf_common.h"
#include "fused_common.h"
#define ONCHIP_NO_AGPR  // one register class for this file's kernels (onchip.h ar / aw)
#include "onchip.h"

using namespace tf;

namespace t2 {

using namespace oc;


// ----------------------------------------------------------------------------------- LDS maps (bytes)
// branch workgroup
// dense image compact (k unpermuted: the K <= 16 MFMA reads k = 4g .. 4g + 3 at byte 8g), which pays for 32-byte
// padding of the v / out_proj images (ds_read_b128 fragment reads conflict-free in gfx950 banking)
constexpr int LDDN = 24 * 2, LDVO = LD64 + 16;
constexpr int B_IMG_D = 0;                         // [64][32]  dense (K = din padded to 32)
constexpr int B_IMG_V = B_IMG_D + 64 * LDDN;       // [64][64]  in_proj rows 128..191 (v)
constexpr int B_IMG_O = B_IMG_V + 64 * LDVO;       // [64][64]  out_proj
constexpr int B_IMG_F1 = B_IMG_O + 64 * LDVO;      // [16][64]  ffn.0 (6 real rows)
constexpr int B_IMG_F2 = B_IMG_F1 + 16 * LD64;     // [64][32]  ffn.3 (6 real columns)
constexpr int B_H0 = B_IMG_F2 + 64 * LD32;         // tile64: h0 = gelu(dense)          (X of dWv)
constexpr int B_A = B_H0 + 16384;                  // tile64: a = att_dropout(v)         (X of dWo)
constexpr int B_X1N = B_A + 16384;                 // tile64: LN1 output                 (X of dWf1)
constexpr int B_DF3 = B_X1N + 16384;               // tile64: d(ffn.3 out)               (dY of dWf2)
constexpr int B_DO = B_DF3 + 16384;                // tile64: d(out_proj out)            (dY of dWo)
constexpr int B_DV = B_DO + 16384;                 // tile64: d(v)                       (dY of dWv)
constexpr int B_DZ0 = B_DV + 16384;                // tile64: d(dense pre-activation)    (dY of dWd)
constexpr int B_XIN = B_DZ0 + 16384;               // tile16: branch input               (X of dWd)
constexpr int B_F2 = B_XIN + 4096;                 // tile16: drop(gelu(ffn.0 out))      (X of dWf2)
constexpr int B_DF0 = B_F2 + 4096;                 // tile16: d(ffn.0 pre-activation)    (dY of dWf1)
constexpr int B_NVEC = 648;                        // 10 x 64 vectors + ffn.0 bias (8 slots, 6 real)
constexpr int B_VEC = B_DF0 + 4096;                // fp32 [648] bias / LayerNorm parameters
// The LayerNorm gradient column sums (6 x 64, produced wave-locally during the backward) are summed over
// the 8 waves as integer quanta in fp64 LDS atomics (onchip.h lds_addq: exact) into DBL; the update reads each
// sum straight into the register of the thread that owns the entry (vec_entry), which zeroes the slot again.
// Integer addition makes the 8-way sum independent of the order the waves arrive in by construction, so a
// client's trajectory is bit-reproducible whatever launch or rank trains it (fp32 LDS atomics were not: ~1e-4
// drift per round; fp64 ones only while the partials spanned < 2^29).  (The bias gradients never touch LDS: they
// are MFMA column sums in the registers of the waves that own those entries.)
constexpr int B_NLN = 6 * 64;
constexpr int B_DBL = B_VEC + B_NVEC * 4;          // fp64 [384]: G1 B1 G2 B2 G3 B3
constexpr int B_DBL_BYTES = B_NLN * 8;
constexpr int B_MISC = B_DBL + B_DBL_BYTES;        // u32 [8] per-wave abort words, then the progress counters
constexpr int B_CNT_A = B_MISC + 32;               // u32: waves past their out_proj backward (DO / DV stored, Wo read)
constexpr int B_CNT_B = B_MISC + 36;               // u32: waves past their whole backward (DZ0 stored, Wv read)
constexpr int B_CNT_C = B_MISC + 40;               // u32: waves past their ffn backward (DF3 / DF0 stored)
constexpr int B_TOTAL = B_MISC + 64;
// vector segments (x64 floats) of VEC
enum { VS_DB = 0, VS_VB, VS_OB, VS_G1, VS_B1, VS_F2B, VS_G2, VS_B2, VS_G3, VS_B3 };
constexpr int VS_F1B = 640;  // ffn.0 bias (6 real)

// head workgroup
// head image row strides (bytes): rows padded by 16 elements (32 B), so the fragment reads are conflict-free in
// gfx950 banking (wfrag ds_read_b128 4 -> 0 extra cycles, wtfrag 4 / 6 -> 2; tools/dbg/lds_banks.py,
// profiles/ab_r5_img_pad.log); the head's LDS map has the room
constexpr int HLD1 = LD128 + 16, HLD2 = LD64 + 16;
constexpr int H_IMG_W1 = 0;                        // [64][128] fc1
constexpr int H_IMG_W2 = H_IMG_W1 + 64 * HLD1;     // [32][64]  fc2
constexpr int H_CAT = H_IMG_W2 + 32 * HLD2;        // tile128: cat(vitals, labs)     (X of dWf1)
constexpr int H_A1 = H_CAT + 32768;                // tile64:  drop(gelu(fc1))       (X of dWf2)
constexpr int H_DZ1 = H_A1 + 16384;                // tile64:  d(fc1 pre-activation) (dY of dWf1)
constexpr int H_DZ2 = H_DZ1 + 16384;               // tile32:  d(fc2 pre-activation) (dY of dWf2)
constexpr int H_NVEC = 132;                        // fc1.b 64 | fc2.b 32 | output.w 32 | output.b 1
constexpr int H_VEC = H_DZ2 + 8192;
constexpr int H_PART = H_VEC + H_NVEC * 4;         // fp32 [8 waves][132] per-wave column sums (their gradients)
constexpr int H_LOSS = H_PART + 8 * H_NVEC * 4;    // fp32 [8] per-wave loss partials, then u32 [8] their abort flags
constexpr int H_CNT = H_LOSS + 64;                 // u32: critical waves past their d(cat) hand-off (4 per step)
constexpr int H_TOTAL = H_CNT + 16;
enum { HV_B1 = 0, HV_B2 = 64, HV_WO = 96, HV_BO = 128 };

constexpr int SMEM_CORE = B_TOTAL > H_TOTAL ? B_TOTAL : H_TOTAL;
// the stamped instantiation (tf2_stamps.hip) times its phases into an LDS tail (onchip.h StampOn); the production
// kernel gets the empty Stamp
#ifdef TF2_STAMPS
using Stamp = StampOn<SMEM_CORE>;
constexpr int SMEM = SMEM_CORE + ST_BYTES;
#else
using Stamp = StampOff;
constexpr int SMEM = SMEM_CORE;
#endif
static_assert(SMEM <= 160 * 1024, "LDS budget");

// ------------------------------------------------------------------- per-client workspace (bytes)
// (the hand-off payloads travel as tagged granules in the per-call zeroed sync block: onchip.h gr_put / gr_get)
// Head: Adam moments of its register-resident weights, slab [slot][thread] of float4 (MOM_SLOTS slots: m and v
// of the 4 fc1 tiles, then the remaining moments), loaded in one batch of sc1 loads ahead of the update phase and
// stored back after it.
// Branch: the compact entries' moments (CMP_SLOTS slots [slot][thread]), then the v / out_proj block UNITS: unit
// 2 w + u (u = 0 out_proj, 1 in_proj.v) is the 2 x 2 tile block (Ta, Tb) of wave w's index w4 = w & 3, stored as
// [unit][12][lane] float4 = m of its 4 tiles, v, then the fp32 master weights p — in memory, not registers, so
// whichever wave is free may update a block (see br_update).
constexpr int MOM_SLOTS = 11;
constexpr long WS_MOM = 0;
constexpr long MOM_WG_BYTES = (long)MOM_SLOTS * NTH * 16;
constexpr int CMP_SLOTS = 1;
constexpr long BR_UNITS = (long)CMP_SLOTS * NTH * 16;
// then the leaders' SMALL units: leader w4's dense / ffn.3 / ffn.0 weight tiles (4 elements per lane each), [w4][9]
// [lane] float4 = m of the three tiles, v, then p
constexpr long BR_SMALL = BR_UNITS + 8L * 12 * 64 * 16;
constexpr long BR_WG_BYTES = BR_SMALL + 4L * 9 * 64 * 16;
constexpr long WS_MOM2 = WS_MOM + MOM_WG_BYTES + 2 * BR_WG_BYTES;   // head half H1's copy of the head's moments
constexpr long WS_BYTES = WS_MOM2 + MOM_WG_BYTES;  // head half H0, vitals branch, labs branch, head half H1

// branch LayerNorm column sums -> fp64 accumulator k of DBL (order G1 B1 G2 B2 G3 B3)
__device__ __forceinline__ void ln_colsum(uchar* smem, int k, const float (&x)[16], int lane) {
  float s;
  const int f = colsum64(x, lane, s);
  lds_addq(smem + B_DBL, 64 * k + f, s);
}
__host__ __device__ constexpr int ln_seg(int k) { return k < 2 ? VS_G1 + k : VS_G2 + (k - 2); }
static_assert(ln_seg(0) == VS_G1 && ln_seg(1) == VS_B1 && ln_seg(2) == VS_G2 && ln_seg(3) == VS_B2 &&
              ln_seg(4) == VS_G3 && ln_seg(5) == VS_B3, "DBL order");

// dropout keep bits of features 16t + 4g + i (bit 4t + i), hash pairs as tf::keep
__device__ __forceinline__ uint32_t mask16(uint32_t key, uint32_t layer, int r, int g, uint32_t thr) {
  uint32_t m = 0;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint32_t x = hash3(key, layer, (uint32_t)r, (uint32_t)(8 * t + 2 * g + h));
      m |= ((x & 0xFFFFu) >= thr ? 1u : 0u) << (4 * t + 2 * h);
      m |= ((x >> 16) >= thr ? 1u : 0u) << (4 * t + 2 * h + 1);
    }
  }
  return m;
}


// Ablation switches of the diagnostic build (compile-time TF2_ABL bits, set through the AFL_TF2_ABL
// environment variable when building tf2_stamps.hip): skip one piece of work per step to price it
// (numerics are wrong then; timing only).  Always false in the production kernel.
enum { ABL_U3 = 1, ABL_UADAM = 2, ABL_UDW = 4, ABL_COLSUM = 8, ABL_HEADUPD = 16, ABL_U1 = 32 };
#if defined(TF2_STAMPS) && defined(TF2_ABL)
#define ABL(K, b) ((TF2_ABL & (b)) != 0)
#else
#define ABL(K, b) false
#endif

// =============================================================================== branch workgroup
template <int BR>
struct BrK {
  static constexpr BrOff o = BR == 0 ? OV : OL;
  static constexpr int din = BR == 0 ? D_V : D_L;
  static constexpr int xoff = BR == 0 ? 0 : D_V;
  // (the dense, ffn.0 and ffn.3 weights are the leaders' small units: smu_elem gives their image positions)
  static constexpr Mat MV{o.inproj_w + 128 * 64, 64, 64, B_IMG_V, LDVO};
  static constexpr Mat MO{o.out_w, 64, 64, B_IMG_O, LDVO};
  // the v (lo) or out_proj block matrix, built from constants (a `lo ? MV : MO` lvalue select would
  // odr-use the static members and load them from memory, defeating the constant folding of n_real / k_real)
  static __device__ __forceinline__ Mat vo(bool lo) {
    return Mat{lo ? MV.off : MO.off, 64, 64, lo ? B_IMG_V : B_IMG_O, LDVO};
  }
  // VEC segment -> flat parameter offset
  static __device__ __forceinline__ int vec_param(int e) {
    if (e >= VS_F1B) return e - VS_F1B < FF ? o.ff0_b + (e - VS_F1B) : -1;
    const int s = e >> 6, i = e & 63;  // (a runtime-indexed array would live in scratch)
    const int b = s == 0 ? o.dense_b : s == 1 ? o.inproj_b + 128 : s == 2 ? o.out_b : s == 3 ? o.ln1_w
                : s == 4 ? o.ln1_b : s == 5 ? o.ff3_b : s == 6 ? o.ln2_w : s == 7 ? o.ln2_b : s == 8 ? o.bn_w : o.bn_b;
    return b + i;
  }
};

// values the backward needs from the forward, kept in registers (T layout).  The normalised LayerNorm
// outputs and gelu' are kept as bf16 pairs (the precision the backward's GEMM operands have anyway):
// fp32 copies of all four would not fit beside the optimizer state in the 256-register budget.
struct Saved {
  uint32_t xh1[8], xh2[8], gp[8];
  float rstd1, rstd2;
  uint32_t m1, m2, matt;
  float gk[4];  // drop'(.) * gelu'(ffn.0 out) of features 4g + i
};
__device__ __forceinline__ void save16(uint32_t (&d)[8], const float (&x)[16]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) d[k] = pk2(x[2 * k], x[2 * k + 1]);
}
__device__ __forceinline__ void load16(float (&x)[16], const uint32_t (&d)[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    x[2 * k] = __uint_as_float(d[k] << 16);
    x[2 * k + 1] = __uint_as_float(d[k] & 0xFFFF0000u);
  }
}

// Optimizer state of one branch lane (register-resident, see ar/aw; the v / out_proj blocks' weights and moments live
// in the workspace units, see br_update):
//  * cmp: NCMP "compact" entries, the bias / LayerNorm vectors (VEC index e < 648).  An entry belongs to the thread
//    whose registers hold its gradient sum at the end of br_update's units (vec_entry), so the vector Adam needs
//    no staging and no barrier: at most two entries per thread, riding in the stages of a unit's Adam (br_update).
//    (The dense, ffn.0 and ffn.3 weights were compact entries too; since round 6 the leaders update them as tiles —
//    br_update, small units.)
constexpr int NCMP = 2;
struct BrState {
  VS cmp[NCMP];
};
// Compact entry (VEC index, or -1) of slot h of thread (wave, lane = 16 g + i16):
//   slot 0  waves 2-7: LayerNorm sum k = wave - 2 (DBL order), feature `lane` — the thread reads accumulator
//           64 k + lane; wave 0, g = 0: ffn.0 bias i16 (wave 0's all-ones MFMA over the DF0 tile);
//   slot 1  the column sums of the wave's all-ones MFMAs, one tile per lane group (every accumulator row of a
//           column holds the same sum): g = 0, 1 the unit's dY tiles Tb, Tb + 1 (out_proj bias on waves 0, 2,
//           in_proj.v bias on waves 4, 6), g = 2 ffn.3 bias tile w4, g = 3 dense bias tile w4 (leaders).
__device__ __forceinline__ int vec_entry(int wave, int lane, int h) {
  const int w4 = wave & 3, g = lane >> 4, i16 = lane & 15;
  const bool lead = wave < 4;
  if (h == 0) {
    if (wave >= 2) return ln_seg(wave - 2) * 64 + lane;
    return wave == 0 && g == 0 && VS_F1B + i16 < B_NVEC ? VS_F1B + i16 : -1;
  }
  if (g < 2) return (w4 & 1) == 0 ? (lead ? VS_OB : VS_VB) * 64 + 16 * (2 * (w4 >> 1) + g) + i16 : -1;
  return lead ? (g == 2 ? VS_F2B : VS_DB) * 64 + 16 * w4 + i16 : -1;
}
// (the last two ffn.0 bias slots are padding)
__device__ __forceinline__ bool vec_real(int e) { return e >= 0 && e < VS_F1B + FF; }

// Every dropout keep-bit of a branch wave's forward for one step, packed into two words:
//   mk0 = m1 (out_proj dropout, 16 bits) | m2 (ffn.3 dropout) << 16;
//   mk1 = matt (attention dropout per head, 4 bits) | kf (ffn.0 dropout of features 4g + i) << 4.
// The branch computes the NEXT step's masks while it waits for the head (the wave is idle there) and
// parks them in two registers, so the ~20 hashes per lane leave the forward's critical path.
template <int BR>
__device__ __forceinline__ void br_masks(uint32_t key, int r, int g, uint32_t& mk0, uint32_t& mk1) {
  const uint32_t ha = hash3(key, 8 * BR + L_ATT, r, 0), hb = hash3(key, 8 * BR + L_ATT, r, 1);
  const uint32_t matt = ((ha & 0xFFFFu) >= THR_P01 ? 1u : 0u) | ((ha >> 16) >= THR_P01 ? 2u : 0u) |
                        ((hb & 0xFFFFu) >= THR_P01 ? 4u : 0u) | ((hb >> 16) >= THR_P01 ? 8u : 0u);
  const uint32_t m1 = mask16(key, 8 * BR + L_D1, r, g, THR_P01), m2 = mask16(key, 8 * BR + L_D2, r, g, THR_P01);
  uint32_t kf = 0u;
  if (g < 2) {
    const uint32_t hd[2] = {hash3(key, 8 * BR + L_DF, r, 2 * g), hash3(key, 8 * BR + L_DF, r, 2 * g + 1)};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t u = (hd[i >> 1] >> ((i & 1) << 4)) & 0xFFFFu;
      kf |= (4 * g + i < FF && u >= THR_P01 ? 1u : 0u) << i;
    }
  }
  mk0 = m1 | (m2 << 16);
  mk1 = matt | (kf << 4);
}

// Fragment pipeline (br_forward, br_backward).  Each sub-phase consumes bf16 weight-image fragments that depend on no
// activation, but the sched_barrier in front of it keeps their ds_reads behind the previous sub-phase's epilogue VALU,
// so every layer boundary exposed one LDS round trip on a latency-bound chain.  The k-step-0 fragments of the NEXT
// sub-phase's first MFMAs (both k-steps where they are small) are therefore issued at the top of the CURRENT one,
// above a fence of their own — in flight under its MFMAs and epilogue — and pinned at its end like bp.f3 (br_bwd_pre),
// so they are neither sunk nor re-read.  The MFMA order is unchanged: results are bit-identical by construction.
// Safe because the forward's images are final between the step's end barrier and this step's update, and in the
// backward a wave reads an image only BEFORE it signals the counter that frees it (ffn.0 / out_proj: A, in_proj.v:
// B): a prefetch inside the same wave's backward is issued even earlier than the read it replaces, and lds_signal
// drains the wave's LDS reads before the count moves.
template <int N, class V>
__device__ __forceinline__ void pin(V (&f)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) asm volatile("" : "+v"(f[i]));
}

template <int BR>
__device__ __forceinline__ void br_forward(uchar* smem, const float (&xin)[4], uint32_t mk0, uint32_t mk1, Saved& sv,
                                           u32x4 (&outp)[2], int lane, int wave) {
  using B = BrK<BR>;
  opq(lane, wave);
  const int g = lane >> 4, r = 16 * wave + (lane & 15);
  const uchar* vg = lane_vec(smem + B_VEC, g);  // (one lane base for every vector read of the phase)
  st4<TK16>(smem + B_XIN, r, g, xin);
  // ---- dense (K = din <= 16 padded to 32) + GELU
  float h0[16];
  s8v pfv[4], pfo[4], pf1[2];  // k-step-0 fragments of v / out_proj, both of ffn.0: loaded one sub-phase ahead
  s4v pf3[4];                  // ffn.3's
  sb();
  {
    const s4v bx = bfrag4(xin);
    f4v acc[4];
    s4v wd[4];
#pragma unroll
    for (int T = 0; T < 4; ++T)
      wd[T] = *(const LDS_AS s4v*)(smem + B_IMG_D + (16 * T + (lane & 15)) * LDDN + 8 * (lane >> 4));
    // (the dense fragments first, the v fragments behind them: LDS returns in order)
    sb();
#pragma unroll
    for (int T = 0; T < 4; ++T) pfv[T] = wfrag(smem + B_IMG_V, LDVO, T, 0, lane);
    sb();
#pragma unroll
    for (int T = 0; T < 4; ++T) acc[T] = mma16(wd[T], bx, Z4);
    float bd[16], gp[16];
    vec16g(bd, vg + VS_DB * 256);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int i = 0; i < 4; i += 2) {
        gf2v g2;
        const gf2v y = gelu2(gf2v{acc[t][i] + bd[4 * t + i], acc[t][i + 1] + bd[4 * t + i + 1]}, g2);
        h0[4 * t + i] = y[0];
        h0[4 * t + i + 1] = y[1];
        gp[4 * t + i] = g2[0];
        gp[4 * t + i + 1] = g2[1];
      }
    save16(sv.gp, gp);
#pragma unroll
    for (int t = 0; t < 4; ++t) st4<TK64>(smem + B_H0, r, 4 * t + g, h0 + 4 * t);
    pin(pfv);
  }
  // ---- v projection, attention dropout per (row, head); at L = 1 softmax == 1, so attn = drop(v)
  float a[16];
  sb();
  {
    s8v w1[4];
#pragma unroll
    for (int T = 0; T < 4; ++T) w1[T] = wfrag(smem + B_IMG_V, LDVO, T, 1, lane);
#pragma unroll
    for (int T = 0; T < 4; ++T) pfo[T] = wfrag(smem + B_IMG_O, LDVO, T, 0, lane);
    sb();
    const s8v b0 = bfrag(h0, 0), b1 = bfrag(h0, 1);
    f4v acc[4];
#pragma unroll
    for (int T = 0; T < 4; ++T) {
      acc[T] = mma(pfv[T], b0, Z4);
      acc[T] = mma(w1[T], b1, acc[T]);
    }
    sv.matt = mk1 & 0xFu;
    float bv[16];
    vec16g(bv, vg + VS_VB * 256);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float m = keepf(INV_K01, sv.matt, t);
#pragma unroll
      for (int i = 0; i < 4; ++i) a[4 * t + i] = (acc[t][i] + bv[4 * t + i]) * m;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) st4<TK64>(smem + B_A, r, 4 * t + g, a + 4 * t);
    pin(pfo);
  }
  // ---- out projection, dropout, residual, LayerNorm 1
  float x1n[16];
  sb();
  {
    s8v w1[4];
#pragma unroll
    for (int T = 0; T < 4; ++T) w1[T] = wfrag(smem + B_IMG_O, LDVO, T, 1, lane);
    pf1[0] = wfrag(smem + B_IMG_F1, LD64, 0, 0, lane);
    pf1[1] = wfrag(smem + B_IMG_F1, LD64, 0, 1, lane);
    sb();
    const s8v b0 = bfrag(a, 0), b1 = bfrag(a, 1);
    f4v acc[4];
#pragma unroll
    for (int T = 0; T < 4; ++T) {
      acc[T] = mma(pfo[T], b0, Z4);
      acc[T] = mma(w1[T], b1, acc[T]);
    }
    sv.m1 = mk0 & 0xFFFFu;
    float bo[16];
    vec16g(bo, vg + VS_OB * 256);
    float x1[16];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int j = 4 * t + i;
        x1[j] = h0[j] + keepf((acc[t][i] + bo[j]) * INV_K01, sv.m1, j);
      }
    sv.rstd1 = ln_fwd2(x1);
    save16(sv.xh1, x1);
    float gm[16], bt[16];
    vec16g(gm, vg + VS_G1 * 256);
    vec16g(bt, vg + VS_B1 * 256);
    affine2(x1n, x1, gm, bt);
#pragma unroll
    for (int t = 0; t < 4; ++t) st4<TK64>(smem + B_X1N, r, 4 * t + g, x1n + 4 * t);
    pin(pf1);
  }
  // ---- ffn.0 (64 -> 6, one output tile) + GELU + dropout
  float f2v[4];
  sb();
  {
#pragma unroll
    for (int T = 0; T < 4; ++T) pf3[T] = wfrag4(smem + B_IMG_F2, LD32, T, lane);
    sb();
    f4v acc = mma(pf1[0], bfrag(x1n, 0), Z4);
    acc = mma(pf1[1], bfrag(x1n, 1), acc);
    const f4v bf = g < 2 ? *(const LDS_AS f4v*)(vg + VS_F1B * 4) : Z4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float gp;
      const float gl = gelu_and_grad(acc[i] + bf[i], gp);
      f2v[i] = keepf(gl * INV_K01, mk1, 4 + i);
      sv.gk[i] = keepf(gp * INV_K01, mk1, 4 + i);
    }
    st4<TK16>(smem + B_F2, r, g, f2v);
    pin(pf3);
  }
  // ---- ffn.3 (6 -> 64, K padded to 32), dropout, residual, LayerNorm 2, LayerNorm 3 (x_bn)
  sb();
  {
    const s4v bf = bfrag4(f2v);
    f4v acc[4];
#pragma unroll
    for (int T = 0; T < 4; ++T) acc[T] = mma16(pf3[T], bf, Z4);
    sv.m2 = mk0 >> 16;
    float b3[16];
    vec16g(b3, vg + VS_F2B * 256);
    float x2[16];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int j = 4 * t + i;
        x2[j] = x1n[j] + keepf((acc[t][i] + b3[j]) * INV_K01, sv.m2, j);
      }
    sv.rstd2 = ln_fwd2(x2);
    save16(sv.xh2, x2);
    float gm[16], bt[16];
    vec16g(gm, vg + VS_G2 * 256);
    vec16g(bt, vg + VS_B2 * 256);
    affine2(x2, x2, gm, bt);
    ln_fwd2(x2);
    vec16g(gm, vg + VS_G3 * 256);
    vec16g(bt, vg + VS_B3 * 256);
    affine2(x2, x2, gm, bt);
    pack16(x2, outp);
  }
}

// The part of the backward that does not depend on d(out): the transposed ffn.3 fragments of its first GEMM, and the
// LayerNorm-3 input xh3 = LN(xh2 * gamma2 + beta2) with its rstd, recomputed from the saved bf16 xh2 (fewer saved registers than keeping the forward's fp32 values, and the
// backward's own bits: the forward normalised the unrounded row).  Run by each wave while it waits for the head's
// hand-off — gamma2 / beta2 and the image change only in the update — and held in registers (25) across the wait.
// (Holding gamma3 too measured inside the noise, gamma2 as well spilled: profiles/ab_tf2_tail.log; in one register
// class gamma3 alone spills the hand-off store offsets and measured -2.8 %: profiles/ab_tf2_regs.log.)
struct BwdPre {
  float xh3[16], rstd3;
  s8v f3[2];  // the transposed ffn.3 image fragments of the backward's first GEMM (final since the last update)
};
__device__ __forceinline__ void br_bwd_pre(const uchar* smem, const Saved& sv, BwdPre& bp, int lane) {
  const uchar* vg = lane_vec(smem + B_VEC, lane >> 4);
  float gm[16], bt[16];
  load16(bp.xh3, sv.xh2);
  vec16g(gm, vg + VS_G2 * 256);
  vec16g(bt, vg + VS_B2 * 256);
  affine2(bp.xh3, bp.xh3, gm, bt);
  bp.rstd3 = ln_fwd2(bp.xh3);
#pragma unroll
  for (int j = 0; j < 16; ++j) asm volatile("" : "+v"(bp.xh3[j]));  // (computed here, not sunk below the wait)
  asm volatile("" : "+v"(bp.rstd3));
  bp.f3[0] = wtfrag<true>(smem + B_IMG_F2, LD32, 0, 0, lane);
  bp.f3[1] = wtfrag<true>(smem + B_IMG_F2, LD32, 0, 1, lane);
  asm volatile("" : "+v"(bp.f3[0]), "+v"(bp.f3[1]));
}

// d(branch output) -> every activation gradient of the branch (wave-local), the dY tiles of the dW
// GEMMs and the column sums of the vector gradients
template <int BR>
__device__ __forceinline__ void br_backward(uchar* smem, const float (&dout)[16], const Saved& sv, const BwdPre& bp,
                                            const AdamK& K, int lane, int wave) {
  opq(lane, wave);
  const int g = lane >> 4, r = 16 * wave + (lane & 15);
  const uchar* vg = lane_vec(smem + B_VEC, g);
  float dr2[16];
  sb();
  {  // LayerNorm 3 and 2 backward (xh3 and rstd3 from br_bwd_pre)
    float gm[16], t[16], dx[16], xh[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) xh[j] = bp.xh3[j];
    const float rstd3 = bp.rstd3;
#pragma unroll
    for (int j = 0; j < 16; ++j) t[j] = dout[j] * xh[j];
    if (!ABL(K, ABL_COLSUM)) ln_colsum(smem, 4, t, lane);
    if (!ABL(K, ABL_COLSUM)) ln_colsum(smem, 5, dout, lane);
    vec16g(gm, vg + VS_G3 * 256);
    ln_bwd2(dx, dout, xh, rstd3, gm);
    load16(xh, sv.xh2);
#pragma unroll
    for (int j = 0; j < 16; ++j) t[j] = dx[j] * xh[j];
    if (!ABL(K, ABL_COLSUM)) ln_colsum(smem, 2, t, lane);
    if (!ABL(K, ABL_COLSUM)) ln_colsum(smem, 3, dx, lane);
    vec16g(gm, vg + VS_G2 * 256);
    ln_bwd2(dr2, dx, xh, sv.rstd2, gm);
  }
  float df0[4];
  s4v pt1[4];          // the transposed ffn.0 fragments, loaded one sub-phase ahead (fragment pipeline, above)
  s8v pto[4], ptv[4];  // the k-step-0 transposed out_proj / in_proj.v fragments
  sb();
  {  // d(ffn.3 out) -> ffn.3 backward (d f2) -> d(ffn.0 pre-activation)
#pragma unroll
    for (int T = 0; T < 4; ++T) pt1[T] = wtfrag4(smem + B_IMG_F1, LD64, T, lane);
    sb();
    float d3[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) d3[j] = keepf(dr2[j] * INV_K01, sv.m2, j);
#pragma unroll
    for (int t = 0; t < 4; ++t) st4<TK64>(smem + B_DF3, r, 4 * t + g, d3 + 4 * t);
    f4v acc = mma(bp.f3[0], bfrag(d3, 0), Z4);
    acc = mma(bp.f3[1], bfrag(d3, 1), acc);
#pragma unroll
    for (int i = 0; i < 4; ++i) df0[i] = acc[i] * sv.gk[i];
    st4<TK16>(smem + B_DF0, r, g, df0);
    pin(pt1);
  }
  lds_signal(smem, B_CNT_C, lane);  // DF3 / DF0 rows stored: the ffn weight tiles may be computed
  float dr1[16];
  sb();
  {  // ffn.0 backward (d x1n) + residual, LayerNorm 1 backward
#pragma unroll
    for (int T = 0; T < 4; ++T) pto[T] = wtfrag<true>(smem + B_IMG_O, LDVO, T, 0, lane);
    sb();
    const s4v bd = bfrag4(df0);
    float dx[16];
#pragma unroll
    for (int T = 0; T < 4; ++T) {
      const f4v acc = mma16(pt1[T], bd, Z4);
#pragma unroll
      for (int i = 0; i < 4; ++i) dx[4 * T + i] = acc[i] + dr2[4 * T + i];
    }
    float t[16], gm[16], xh[16];
    load16(xh, sv.xh1);
#pragma unroll
    for (int j = 0; j < 16; ++j) t[j] = dx[j] * xh[j];
    if (!ABL(K, ABL_COLSUM)) ln_colsum(smem, 0, t, lane);
    if (!ABL(K, ABL_COLSUM)) ln_colsum(smem, 1, dx, lane);
    vec16g(gm, vg + VS_G1 * 256);
    ln_bwd2(dr1, dx, xh, sv.rstd1, gm);
    pin(pto);
  }
  float dv[16];
  sb();
  {  // out_proj backward: d a = d o . Wo ; d v = attention-dropout'(d a)
#pragma unroll
    for (int T = 0; T < 4; ++T) ptv[T] = wtfrag<true>(smem + B_IMG_V, LDVO, T, 0, lane);
    sb();
    float dO[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) dO[j] = keepf(dr1[j] * INV_K01, sv.m1, j);
#pragma unroll
    for (int t = 0; t < 4; ++t) st4<TK64>(smem + B_DO, r, 4 * t + g, dO + 4 * t);
    const s8v b0 = bfrag(dO, 0), b1 = bfrag(dO, 1);
#pragma unroll
    for (int T = 0; T < 4; ++T) {
      f4v acc = mma(pto[T], b0, Z4);
      acc = mma(wtfrag<true>(smem + B_IMG_O, LDVO, T, 1, lane), b1, acc);
      const float m = keepf(INV_K01, sv.matt, T);
#pragma unroll
      for (int i = 0; i < 4; ++i) dv[4 * T + i] = acc[i] * m;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) st4<TK64>(smem + B_DV, r, 4 * t + g, dv + 4 * t);
    pin(ptv);
  }
  lds_signal(smem, B_CNT_A, lane);  // DO / DV rows stored, out_proj image read: its block may be updated
  sb();
  {  // v backward: d h0 = d r1 + d v . Wv ; d z0 = d h0 * gelu'(z0)
    const s8v b0 = bfrag(dv, 0), b1 = bfrag(dv, 1);
    float dz[16], gp[16];
    load16(gp, sv.gp);
#pragma unroll
    for (int T = 0; T < 4; ++T) {
      f4v acc = mma(ptv[T], b0, Z4);
      acc = mma(wtfrag<true>(smem + B_IMG_V, LDVO, T, 1, lane), b1, acc);
#pragma unroll
      for (int i = 0; i < 4; ++i) dz[4 * T + i] = (acc[i] + dr1[4 * T + i]) * gp[4 * T + i];
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) st4<TK64>(smem + B_DZ0, r, 4 * t + g, dz + 4 * t);
  }
  lds_signal(smem, B_CNT_B, lane);  // backward done: DZ0 rows stored, v image read, LayerNorm sums added
}


// compact entry e (< 648: a bias / LayerNorm vector element) of branch BR: flat parameter index (or -1)
template <int BR>
__device__ __forceinline__ int cmp_param(int e) {
  return vec_real(e) ? BrK<BR>::vec_param(e) : -1;
}

// ------------------------------------------------------------------------------ branch weight update
// Block units (workspace, see WS layout): wave index w4 = w & 3 names the 2 x 2 tile block (Ta = 2 (w4 & 1),
// Tb = 2 (w4 >> 1)) of the 64 x 64 out_proj (u = 0) or in_proj.v (u = 1) weight gradient; lane holds 4 elements
// per tile, tile t = 2a + b = (Ta + a, Tb + b): slots j = t (m), 4 + t (v), 8 + t (fp32 weight p).
__device__ __forceinline__ f4v unit_ld(__amdgpu_buffer_rsrc_t rm, int ui, int j, int lane) {
  return __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(rm, (int)BR_UNITS + ((ui * 12 + j) * 64 + lane) * 16,
                                                                        0, 16));
}
__device__ __forceinline__ void unit_st(__amdgpu_buffer_rsrc_t rm, int ui, int j, int lane, f4v v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rm, (int)BR_UNITS + ((ui * 12 + j) * 64 + lane) * 16,
                                         0, 0);
  store_guard();
}
// A thread's vector entries (vec_entry) on their way through a unit's Adam stages: weights (VS registers), moments,
// gradient sums in; new weights out in pn
struct VecAd {
  float m[NCMP], v[NCMP], g[NCMP], pn[NCMP];
};
// Adam on N independent elements in explicit stages (every m / v update, every square root, every reciprocal, every
// weight), so the N sqrt -> rcp -> fma chains overlap, with every contraction written out.  Which products of
// `b2 v + (1 - b2) g g` and `g - keep m` the compiler fuses depends on the code around the call (it moved once:
// profiles/ab_tf2_tail.log), and a trained model must not change with that, so each group of elements has the form
// it compiled to before the forms were pinned (read from the ISA of the commit before, both branch instantiations):
//   elements [0, NA)       m' = fma(c1, fma(-keep, m, g), keep m);  v' = fma(b2, v, g ((1 - b2) g))
//   elements [NA, N - NV)  the same m';                             v' = fma(g, (1 - b2) g, b2 v)
//   elements [N - NV, N)   m' = fma(c1, g - keep m, keep m);        v' = fma(g, (1 - b2) g, b2 v)
//   all                    p' = fma(-(lr_bc1 m'), 1 / fma(rsqrt_bc2, sqrt(v'), eps), p)
// The passes: unit_adam is (16 + NV, 16, NV) — the laggards' v unit with their vector entries (NV = 2), the leaders'
// out_proj unit (NV = 0); ffn_adam, the leaders' ffn.3 / ffn.0 tiles before counter A, is (8, 0, 0): the second form;
// dense_adam, the leaders' dense tile with their vector entries, is (6, 4, 2).  The last NV elements are a thread's
// vector entries, in the form their own pass (vec_adam, until it was folded in here) had pinned for them.  (Until the
// ffn tiles got a pass of their own, the three small tiles were one (14, 4, 2) pass: every element keeps the form it
// had there.)
template <int N, int NA, int NV>
__device__ __forceinline__ void adam_pinned(float (&p)[N], float (&mm)[N], float (&vv)[N], const float (&g)[N],
                                            const AdamK& K) {
#pragma clang fp contract(off)
  float den[N];
#pragma unroll
  for (int e = 0; e < N; ++e) {
    const float mk = mm[e] * K.keep;
    const float d = e < N - NV ? __builtin_fmaf(-K.keep, mm[e], g[e]) : g[e] - mk;
    mm[e] = __builtin_fmaf(K.c1, d, mk);
    const float t = (1.f - fk::B2) * g[e];
    if (e < NA) {
      const float t2 = g[e] * t;
      vv[e] = __builtin_fmaf(fk::B2, vv[e], t2);
    } else {
      const float u = fk::B2 * vv[e];
      vv[e] = __builtin_fmaf(g[e], t, u);
    }
  }
#pragma unroll
  for (int e = 0; e < N; ++e) den[e] = __builtin_amdgcn_sqrtf(vv[e]);
#pragma unroll
  for (int e = 0; e < N; ++e) den[e] = __builtin_amdgcn_rcpf(__builtin_fmaf(K.rsqrt_bc2, den[e], K.eps));
#pragma unroll
  for (int e = 0; e < N; ++e) {
    const float lm = K.lr_bc1 * mm[e];
    p[e] = __builtin_fmaf(-lm, den[e], p[e]);
  }
}
// Adam on the 16 elements of a unit (p, m, v in U, gradients acc[a][b] of tile 2a + b) and, when NV > 0, on the
// thread's NV vector entries in the same stages: two more independent chains there instead of a dependent
// sqrt -> rcp -> fma chain of their own at the end of the step
template <int NV>
__device__ __forceinline__ void unit_adam(f4v (&U)[12], const f4v (&acc)[2][2], const AdamK& K, VS (&pa)[NCMP],
                                          VecAd& x) {
  static_assert(NV == 0 || NV == NCMP, "all of the thread's vector entries or none");
  float p[16 + NV], mm[16 + NV], vv[16 + NV], g[16 + NV];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      mm[4 * t + i] = U[t][i];
      vv[4 * t + i] = U[4 + t][i];
      p[4 * t + i] = U[8 + t][i];
      g[4 * t + i] = acc[t >> 1][t & 1][i];
    }
#pragma unroll
  for (int h = 0; h < NV; ++h) {
    mm[16 + h] = x.m[h];
    vv[16 + h] = x.v[h];
    p[16 + h] = ar(pa[h].p);
    g[16 + h] = x.g[h];
  }
  adam_pinned<16 + NV, 16, NV>(p, mm, vv, g, K);
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      U[t][i] = mm[4 * t + i];
      U[4 + t][i] = vv[4 * t + i];
      U[8 + t][i] = p[4 * t + i];
    }
#pragma unroll
  for (int h = 0; h < NV; ++h) {
    x.m[h] = mm[16 + h];
    x.v[h] = vv[16 + h];
    x.pn[h] = p[16 + h];
    pa[h].p = aw(p[16 + h]);
  }
}
// the unit's new bf16 weights into its image (rows n = 16 (Tb + b) + i16, permuted k chunk of tile Ta + a)
__device__ __forceinline__ void unit_img(uchar* smem, const Mat& M, int Ta, int Tb, int lane, const u32x2v (&w)[4]) {
  const int i16 = lane & 15, g4 = 4 * (lane >> 4);
#pragma unroll
  for (int t = 0; t < 4; ++t)
    *(LDS_AS u32x2v*)(smem + M.img + (16 * (Tb + (t & 1)) + i16) * M.ld + pcol(16 * (Ta + (t >> 1)) + g4) * 2) = w[t];
}
__device__ __forceinline__ void unit_pack(const f4v (&U)[12], u32x2v (&w)[4]) {
#pragma unroll
  for (int t = 0; t < 4; ++t) w[t] = u32x2v{pk2(U[8 + t][0], U[8 + t][1]), pk2(U[8 + t][2], U[8 + t][3])};
}
// dW^T of a unit over all 128 rows: acc[a][b] = X tile Ta + a  x  dY tile Tb + b; bias column sums of dY tiles
// Tb, Tb + 1 (the all-ones X fragment) when `bias`
__device__ __forceinline__ void unit_dw(const uchar* X, const uchar* DY, int Ta, int Tb, int lane, bool bias,
                                        f4v (&acc)[2][2], f4v (&bs)[2]) {
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = Z4;
  bs[0] = bs[1] = Z4;
  // (the all-ones operand from an opaque SGPR, materialised here: hoisted out of the step loop it is spilled)
  uint32_t o1 = 0x3F803F80u;
  asm volatile("" : "+s"(o1));
  const s8v one = __builtin_bit_cast(s8v, u32x4{o1, o1, o1, o1});
#pragma unroll  // (fully unrolled: the fragment reads of later k-steps overlap earlier MFMAs, +2.2 %)
  for (int s = 0; s < 4; ++s) {
    const s8v x0 = tfrag<TK64>(X, 32 * s, Ta, lane), x1 = tfrag<TK64>(X, 32 * s, Ta + 1, lane);
    const s8v y0 = tfrag<TK64>(DY, 32 * s, Tb, lane), y1 = tfrag<TK64>(DY, 32 * s, Tb + 1, lane);
    acc[0][0] = mma(x0, y0, acc[0][0]);
    acc[0][1] = mma(x0, y1, acc[0][1]);
    acc[1][0] = mma(x1, y0, acc[1][0]);
    acc[1][1] = mma(x1, y1, acc[1][1]);
    if (bias) {
      bs[0] = mma(one, y0, bs[0]);
      bs[1] = mma(one, y1, bs[1]);
    }
  }
}

// Small units: leader w4 owns its dense tile (k 0..15, n tile w4), ffn.3 tile (n tile w4, k 0..15) and ffn.0 k tile
// w4 (n 0..15) — the weight-gradient tiles it computes (lane element (k = 16 T + 4g + i, n = 16 Tn + i16)); tile s
// of the unit: 0 dense, 1 ffn.3, 2 ffn.0; slots s (m), 3 + s (v), 6 + s (p).  Padding elements (k >= din, ffn k >= 6,
// ffn.0 n >= 6) keep p = 0: their inputs / gradients are exactly zero, so Adam leaves them there.
__device__ __forceinline__ f4v smu_ld(__amdgpu_buffer_rsrc_t rm, int w4, int j, int lane) {
  return __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(rm, (int)BR_SMALL + ((w4 * 9 + j) * 64 + lane) * 16,
                                                                        0, 16));
}
__device__ __forceinline__ void smu_st(__amdgpu_buffer_rsrc_t rm, int w4, int j, int lane, f4v v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rm, (int)BR_SMALL + ((w4 * 9 + j) * 64 + lane) * 16,
                                         0, 0);
  store_guard();
}
// (flat parameter index, bf16 image byte offset) of element i of small tile s of leader w4's lane, or pi = -1
template <int BR>
__device__ __forceinline__ void smu_elem(int s, int w4, int lane, int i, int& pi, int& img) {
  using B = BrK<BR>;
  constexpr int din = BrK<BR>::din;
  const int g = lane >> 4, i16 = lane & 15;
  if (s == 0) {  // dense W[n][k], n = 16 w4 + i16, k = 4g + i; image compact, k unpermuted
    const int n = 16 * w4 + i16, k = 4 * g + i;
    pi = k < din ? B::o.dense_w + n * din + k : -1;
    img = B_IMG_D + n * LDDN + k * 2;
  } else if (s == 1) {  // ffn.3 W[n][k], n = 16 w4 + i16, k = 4g + i < 6
    const int n = 16 * w4 + i16, k = 4 * g + i;
    pi = k < FF ? B::o.ff3_w + n * FF + k : -1;
    img = B_IMG_F2 + n * LD32 + pcol(k) * 2;
  } else {  // ffn.0 W[n][k], n = i16 < 6, k = 16 w4 + 4g + i
    const int n = i16, k = 16 * w4 + 4 * g + i;
    pi = n < FF ? B::o.ff0_w + n * 64 + k : -1;
    img = B_IMG_F1 + n * LD64 + pcol(k) * 2;
  }
}
// Adam on a leader's ffn.3 and ffn.0 tiles (F = {m1 m2, v1 v2, p1 p2}: small-unit slots 1, 2 / 4, 5 / 7, 8), gradients
// g3 / g1: the pass the leaders run before counter A (br_update)
__device__ __forceinline__ void ffn_adam(f4v (&F)[6], const f4v& g3, const f4v& g1, const AdamK& K) {
  float p[8], mm[8], vv[8], g[8];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      mm[4 * s + i] = F[s][i];
      vv[4 * s + i] = F[2 + s][i];
      p[4 * s + i] = F[4 + s][i];
      g[4 * s + i] = s == 0 ? g3[i] : g1[i];
    }
  adam_pinned<8, 0, 0>(p, mm, vv, g, K);
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      F[s][i] = mm[4 * s + i];
      F[2 + s][i] = vv[4 * s + i];
      F[4 + s][i] = p[4 * s + i];
    }
}
// Adam on a leader's dense tile (D = {m, v, p}: small-unit slots 0, 3, 6; gradient gd) and on the thread's vector
// entries in the same stages (unit_adam)
__device__ __forceinline__ void dense_adam(f4v (&D)[3], const f4v& gd, const AdamK& K, VS (&pa)[NCMP], VecAd& x) {
  constexpr int N = 4 + NCMP;
  float p[N], mm[N], vv[N], g[N];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    mm[i] = D[0][i];
    vv[i] = D[1][i];
    p[i] = D[2][i];
    g[i] = gd[i];
  }
#pragma unroll
  for (int h = 0; h < NCMP; ++h) {
    mm[4 + h] = x.m[h];
    vv[4 + h] = x.v[h];
    p[4 + h] = ar(pa[h].p);
    g[4 + h] = x.g[h];
  }
  adam_pinned<N, 4, NCMP>(p, mm, vv, g, K);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    D[0][i] = mm[i];
    D[1][i] = vv[i];
    D[2][i] = p[i];
  }
#pragma unroll
  for (int h = 0; h < NCMP; ++h) {
    x.m[h] = mm[4 + h];
    x.v[h] = vv[4 + h];
    x.pn[h] = p[4 + h];
    pa[h].p = aw(p[4 + h]);
  }
}
// the new weights p of small tile s into its image (4 consecutive (permuted) k per lane: one 8-byte store)
template <int BR>
__device__ __forceinline__ void smu_img(uchar* smem, int s, const f4v& p, int w4, int lane) {
  int pi, img;
  smu_elem<BR>(s, w4, lane, 0, pi, img);
  *(LDS_AS u32x2v*)(smem + img) = u32x2v{pk2(p[0], p[1]), pk2(p[2], p[3])};
}

// Weight gradients + Adam for one step, started by each wave as soon as its own backward is done — no barrier
// between the backward and the weight-gradient work.  The waves of a SIMD pair run the same chain and the arbiter
// favours the older one, so waves 0-3 ("leaders") reach this point ~2.5 us before waves 4-7 ("laggards", the
// step's critical path).  Each wave starts what its inputs allow, tracked by progress counters (every wave signals
// them from its backward):
//   leaders   counter C (every wave's ffn.3 / ffn.0 dY rows): the ffn.3 tile w4 and ffn.0 k tile w4 weight
//             gradients and the ffn.3 / ffn.0 bias sums, then — still before A, at priority 0 — the abort decision,
//             Adam on those two tiles (ffn_adam), their images and their workspace stores: work that used to follow
//             the barrier, then counter A, now done while the laggards are still in their backward; then counter A
//             (every wave's out_proj dY rows, the out_proj image no longer read): their out_proj unit — dW over the
//             128 rows, Adam on the workspace copy (p, m, v), image, bias sums; then counter B (every wave's dense dY
//             rows): the dense tile w4 and its bias sums, and Adam on that tile (dense_adam), its image and stores;
//   laggards  counter A (the v unit's dY rows): their in_proj.v unit, whose new bf16 weights wait for counter B (the
//             v image is read until the end of every wave's backward).
// The small unit (the dense / ffn.3 / ffn.0 tiles of a leader) is workspace-resident like the blocks.  Its ffn tiles
// are updated before A because nothing they need comes later: their gradients are complete ~0.4 us after C, and C
// also frees their images (ffn.3^T is read in br_bwd_pre, ffn.0^T before each wave's C signal).  Behind A, as part of
// one 14-element pass with the dense tile, they were 8 sqrt -> rcp -> fma chains, two image writes and six stores of
// the leaders' post-A tail, at priority 2 on the SIMD the critical laggard needs: +2.2 % rounds/s for moving them
// (profiles/ab_tf2_update_tail.log; also there, rejected: one Adam pass for out_proj + dense + vector entries after
// B, -0.4 % alone, and the laggards' abort read joined with unit_dw's first fragment reads, inside the noise).
// Inside the last Adam pass of each role (laggards: the v unit's, leaders: the dense tile's) every wave also runs Adam
// on the vector entries it owns (the 648 bias / LayerNorm elements, at most 2 per thread,
// profiles/ab_tf2_frag_pipeline.log): an entry belongs to the thread whose registers hold its gradient sum — a column
// of one of the wave's all-ones MFMA accumulators, or the LayerNorm accumulator the thread reads (vec_entry) — so
// nothing is staged through LDS and the only barrier after the units is the step's end barrier.  (Before, the sums
// went to an fp32 staging array behind one barrier and were read back by thread e % 512 behind a second: 0.8 us of
// every wave's step; and 5 entries per thread when the small weights were vector entries too: +3.6 %,
// profiles/ab_tf2_r6_update.log.)  The abort decision (a NaN loss anywhere in the batch) is taken by every wave before
// it updates anything: by the laggards after counter A, by the leaders after counter C already — all eight abort words
// are final once every wave has passed C, because a wave writes its word before br_backward and its C signal drains
// its LDS operations (the time-out path writes the word before it signals).  Returns false on abort.
// (Measured first: the leaders taking both units after counter A was 1 % slower — A is reached only ~0.2 us
// before B, so the leaders' two units became the tail; profiles/ab_tf2_r6_update.log.)
template <int BR>
__device__ __forceinline__ bool br_update(uchar* smem, BrState& st, const AdamK& K, int lane, int wave, int tid, int step,
                                          __amdgpu_buffer_rsrc_t rm, Stamp& stp, gu32* tmo) {
  using B = BrK<BR>;
  opq(lane, wave);
  asm volatile("" : "+v"(tid));
  const int w4 = wave & 3, g = lane >> 4;
  const bool lead = wave < 4;
  const uint32_t all = 8u * (uint32_t)step;
  LDS_AS uint32_t* abort_w = ldsu(smem, B_MISC);
  const int Ta = 2 * (w4 & 1), Tb = 2 * (w4 >> 1);
  const bool do_bias = (w4 & 1) == 0;  // one of the two units that read dY tiles Tb, Tb + 1
  f4v bsu[2] = {Z4, Z4};               // the unit's bias sums (out_proj on leaders, v on laggards)
  f4v as = Z4, bd = Z4, a3 = Z4, af1 = Z4, b3 = Z4, b1 = Z4;  // leaders: dense / ffn.3 / ffn.0 tiles + bias sums
  const int ui = 2 * w4 + (lead ? 0 : 1);
  f4v U[12];
#pragma unroll
  for (int j = 0; j < 12; ++j) U[j] = unit_ld(rm, ui, j, lane);
  const f4v cmom = mom_ld(rm, 0, tid);  // the vector entries' moments m0 m1 v0 v1 (in flight over the waits below)
  uint32_t o1 = 0x3F803F80u;  // (all-ones operand, opaque SGPR: see unit_dw)
  asm volatile("" : "+s"(o1));
  const s8v one = __builtin_bit_cast(s8v, u32x4{o1, o1, o1, o1});
  auto timed_out = [&]() {
    if (lane == 0) __hip_atomic_store(tmo, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return false;
  };
  // the abort decision: the OR of the eight waves' abort words (two 16-byte reads, one LDS round trip)
  auto abort_now = [&]() {
    const u32x4 a = *(const LDS_AS u32x4*)abort_w, b = *(const LDS_AS u32x4*)(abort_w + 4);
    const u32x4 o = a | b;
    return (o[0] | o[1] | o[2] | o[3]) != 0;
  };
  // ---- the vector entries (648 bias / LayerNorm elements), owner-computed: every gradient sum ends in a register of
  // the thread that owns the entry (vec_entry) — the bias sums in the all-ones MFMA accumulators, the LayerNorm sums
  // read (vec_g0) from the fp64 accumulators.  Those are complete at counter A, which the wave has passed then: every
  // ln_colsum of br_backward precedes its wave's lds_signal(B_CNT_A), and the signal drains the wave's LDS operations
  // first; the backward's last VEC read (gamma1) precedes that signal too, so from there on an owner may write its VEC
  // words.  The slot is zeroed by its reader and added to again only after the step's end barrier.  The entries' Adam
  // rides in the stages of a unit's Adam (laggards: unit_adam, whose v bias sums exist after unit_dw; leaders:
  // dense_adam, right after their last input, the dense bias sums) as two more independent chains, and each owner
  // writes its VEC words next to the unit's image: no staging, no barrier, no dependent chain of its own at the end of
  // the step (it cost every wave ~0.4 us there).  Threads without an entry compute on zeros and store nothing.
  VecAd x;
  auto vec_g0 = [&]() {  // (after counter A and the abort decision)
    x.g[0] = b1[0];
    if (wave >= 2) {
      LDS_AS double* q = (LDS_AS double*)(smem + B_DBL) + 64 * (wave - 2) + lane;
      x.g[0] = lds_getq(smem + B_DBL, 64 * (wave - 2) + lane);
      *q = 0.0;
    }
  };
  auto vec_in = [&]() {  // (once the wave's bias sums exist)
    x.g[1] = g == 0 ? bsu[0][0] : g == 1 ? bsu[1][0] : g == 2 ? b3[0] : bd[0];
    x.m[0] = cmom[0], x.m[1] = cmom[1], x.v[0] = cmom[2], x.v[1] = cmom[3];
  };
  auto vec_out = [&]() {
#pragma unroll
    for (int h = 0; h < NCMP; ++h) {
      // (a few VALU per step: kept as per-thread state the two offsets spill, in two register classes and in one:
      // profiles/ab_tf2_tail.log, profiles/ab_tf2_regs.log)
      const int e = vec_entry(wave, lane, h);
      if (vec_real(e)) ldsf(smem, B_VEC)[e] = x.pn[h];
    }
  };
  f4v acc[2][2];
  u32x2v w[4];
  if (!lead) {
    // ---- the laggards: the in_proj.v unit (X = h0, dY = d v).  Its operands are complete at A — only its image write
    // waits for B, the end of every wave's backward — so its weight-gradient MFMAs overlap the last laggard's v backward
    if (!lds_wait(smem, B_CNT_A, all)) return timed_out();
    if (abort_now()) return false;
    stp(4, tid);
    vec_g0();
    if (!ABL(K, ABL_UDW)) unit_dw(smem + B_H0, smem + B_DV, Ta, Tb, lane, do_bias, acc, bsu);
    vec_in();
    if (!ABL(K, ABL_UADAM)) unit_adam<NCMP>(U, acc, K, st.cmp, x);
    unit_pack(U, w);
    // (the v image is read until the end of every wave's backward)
    if (!lds_wait(smem, B_CNT_B, all)) return timed_out();
    unit_img(smem, B::vo(true), Ta, Tb, lane, w);
    if (!ABL(K, ABL_UADAM)) vec_out();
#pragma unroll
    for (int j = 0; j < 12; ++j) unit_st(rm, ui, j, lane, U[j]);
    mom_st(rm, 0, tid, f4v{x.m[0], x.m[1], x.v[0], x.v[1]});
    return true;
  }
  // ---- the leaders.  Their ffn tiles and the Adam of those run below the laggards' backward on the same SIMD (priority
  // 0: +1.9 % against 2, +1.7 % at 1; profiles/ab_tf2_r6_update.log), the out_proj unit after A at the critical
  // priority again
  prio_lo();
  f4v F[6];  // the ffn.3 / ffn.0 slots of the small unit (in flight over the wait for C and the MFMAs, dead at A)
#pragma unroll
  for (int j = 0; j < 6; ++j) F[j] = smu_ld(rm, w4, 3 * (j >> 1) + 1 + (j & 1), lane);
  if (!lds_wait(smem, B_CNT_C, all)) return timed_out();
#pragma unroll  // (fully unrolled: the fragment reads of later k-steps overlap earlier MFMAs, +2.2 %)
  for (int s = 0; s < (ABL(K, ABL_U1) ? 0 : 4); ++s) {
    const s8v y3 = tfrag<TK64>(smem + B_DF3, 32 * s, w4, lane), y1 = tfrag<TK16>(smem + B_DF0, 32 * s, 0, lane);
    a3 = mma(tfrag<TK16>(smem + B_F2, 32 * s, 0, lane), y3, a3);
    af1 = mma(tfrag<TK64>(smem + B_X1N, 32 * s, w4, lane), y1, af1);
    b3 = mma(one, y3, b3);
    if (wave == 0) b1 = mma(one, y1, b1);
  }
  // The abort decision, before anything is written: all eight words are final once every wave has passed C (a wave
  // writes its word before br_backward, and its C signal drains its LDS operations; the time-out path writes the word
  // before it signals), so the leaders need not wait for A to take it.
  if (abort_now()) return false;
  // Adam on the ffn.3 / ffn.0 tiles, their images and their stores, here and not behind A: the gradients are complete,
  // and from C on nobody reads the two images (ffn.3^T is read in br_bwd_pre, ffn.0^T before each wave's C signal, the
  // forward's reads ended long before) — so this runs in the leaders' wait for A, at priority 0, instead of on the
  // laggards' SIMDs in the step's tail.
  if (!ABL(K, ABL_U3)) ffn_adam(F, a3, af1, K);
  smu_img<BR>(smem, 1, F[4], w4, lane);
  smu_img<BR>(smem, 2, F[5], w4, lane);
#pragma unroll
  for (int j = 0; j < 6; ++j) smu_st(rm, w4, 3 * (j >> 1) + 1 + (j & 1), lane, F[j]);
  if (!lds_wait(smem, B_CNT_A, all)) return timed_out();
  prio_hi();
  stp(4, tid);
  vec_g0();
  // the out_proj unit (X = a, dY = d o): its image is free since A
  if (!ABL(K, ABL_UDW)) unit_dw(smem + B_A, smem + B_DO, Ta, Tb, lane, do_bias, acc, bsu);
  if (!ABL(K, ABL_UADAM)) unit_adam<0>(U, acc, K, st.cmp, x);
  unit_pack(U, w);
  unit_img(smem, B::vo(false), Ta, Tb, lane, w);
#pragma unroll
  for (int j = 0; j < 12; ++j) unit_st(rm, ui, j, lane, U[j]);
  // the dense tile (its dY rows are complete at B); its slots' loads overlap the wait for B and the MFMAs.  Its image
  // is free: it is read only by the forward.
  f4v D[3];
#pragma unroll
  for (int s = 0; s < 3; ++s) D[s] = smu_ld(rm, w4, 3 * s, lane);
  if (!lds_wait(smem, B_CNT_B, all)) return timed_out();
#pragma unroll  // (fully unrolled: the fragment reads of later k-steps overlap earlier MFMAs, +2.2 %)
  for (int s = 0; s < (ABL(K, ABL_U1) ? 0 : 4); ++s) {
    const s8v yd = tfrag<TK64>(smem + B_DZ0, 32 * s, w4, lane);
    as = mma(tfrag<TK16>(smem + B_XIN, 32 * s, 0, lane), yd, as);
    bd = mma(one, yd, bd);
  }
  vec_in();
  if (!ABL(K, ABL_U3)) dense_adam(D, as, K, st.cmp, x);
  smu_img<BR>(smem, 0, D[2], w4, lane);
  if (!ABL(K, ABL_U3)) vec_out();
#pragma unroll
  for (int s = 0; s < 3; ++s) smu_st(rm, w4, 3 * s, lane, D[s]);
  mom_st(rm, 0, tid, f4v{x.m[0], x.m[1], x.v[0], x.v[1]});
  return true;
}

// fresh Adam state (torch.optim.Adam is re-created every round, client.py:78): zero moment slab
__device__ __forceinline__ void mom_zero(__amdgpu_buffer_rsrc_t rm, int tid) {
#pragma unroll
  for (int k = 0; k < MOM_SLOTS; ++k) mom_st(rm, k, tid, Z4);
}

template <int BR>
__device__ __forceinline__ void br_init(uchar* smem, BrState& st, const float* P, __amdgpu_buffer_rsrc_t rm, int lane,
                                        int wave, int tid) {
  using B = BrK<BR>;
#pragma unroll
  for (int k = 0; k < CMP_SLOTS; ++k) mom_st(rm, k, tid, Z4);
  {  // wave w: unit 2 (w & 3) + (w >> 2) (every unit once): p from the parameters -> workspace + bf16 image, m = v = 0
    const int w4 = wave & 3, u = wave >> 2, Ta = 2 * (w4 & 1), Tb = 2 * (w4 >> 1);
    const Mat M = B::vo(u == 1);
    const int i16 = lane & 15, g4 = 4 * (lane >> 4);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int n = 16 * (Tb + (t & 1)) + i16, k0 = 16 * (Ta + (t >> 1)) + g4;
      const float* src = P + M.off + n * M.k_real + k0;  // (a client's parameter row is not 16-byte aligned)
      const f4v p = {src[0], src[1], src[2], src[3]};
      unit_st(rm, 2 * w4 + u, t, lane, Z4);
      unit_st(rm, 2 * w4 + u, 4 + t, lane, Z4);
      unit_st(rm, 2 * w4 + u, 8 + t, lane, p);
      *(LDS_AS u32x2v*)(smem + M.img + n * M.ld + pcol(k0) * 2) = u32x2v{pk2(p[0], p[1]), pk2(p[2], p[3])};
    }
  }
  if (wave < 4) {  // leader w4's small unit: p from the parameters (0 for padding) -> workspace + images, m = v = 0
    f4v S[9];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      S[s] = S[3 + s] = Z4;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int pi, img;
        smu_elem<BR>(s, wave, lane, i, pi, img);
        S[6 + s][i] = pi >= 0 ? P[pi] : 0.f;
      }
    }
#pragma unroll
    for (int s = 0; s < 3; ++s) smu_img<BR>(smem, s, S[6 + s], wave, lane);
#pragma unroll
    for (int j = 0; j < 9; ++j) smu_st(rm, wave, j, lane, S[j]);
  }
#pragma unroll
  for (int h = 0; h < NCMP; ++h) {
    const int e = vec_entry(wave, lane, h);
    float p0 = 0.f;
    if (e >= 0) {
      const int pi = cmp_param<BR>(e);
      p0 = pi >= 0 ? P[pi] : 0.f;
      ldsf(smem, B_VEC)[e] = p0;
    }
    st.cmp[h] = VS{aw(p0)};
  }
}

template <int BR>
__device__ __forceinline__ void br_fini(const BrState& st, float* P, __amdgpu_buffer_rsrc_t rm, int lane, int wave,
                                        int tid) {
  using B = BrK<BR>;
  opq(lane, wave);  // (addresses recomputed here, not carried from br_init across the step loop)
  {  // the units' weights (stored by the waves that updated them: wait for every store before reading back)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int w4 = wave & 3, u = wave >> 2, Ta = 2 * (w4 & 1), Tb = 2 * (w4 >> 1);
    const Mat M = B::vo(u == 1);
    const int i16 = lane & 15, g4 = 4 * (lane >> 4);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int n = 16 * (Tb + (t & 1)) + i16, k0 = 16 * (Ta + (t >> 1)) + g4;
      const f4v p = unit_ld(rm, 2 * w4 + u, 8 + t, lane);
      float* dst = P + M.off + n * M.k_real + k0;
#pragma unroll
      for (int i = 0; i < 4; ++i) dst[i] = p[i];
      store_guard();  // (merged into one 16-byte store: the next unit's load must not be its very next instruction)
    }
  }
  if (wave < 4) {  // leader w4's small unit (its own stores)
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      const f4v p = smu_ld(rm, wave, 6 + s, lane);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int pi, img;
        smu_elem<BR>(s, wave, lane, i, pi, img);
        if (pi >= 0) P[pi] = p[i];
      }
      store_guard();
    }
  }
#pragma unroll
  for (int h = 0; h < NCMP; ++h) {
    const int e = vec_entry(wave, lane, h);
    if (e >= 0) {
      const int pi = cmp_param<BR>(e);
      if (pi >= 0) P[pi] = ar(st.cmp[h].p);
    }
  }
}

// this lane's 4 input features (4g + i) of row r = 16 wave + (lane & 15) of the batch starting at b0 of epoch e
template <int BR>
__device__ __forceinline__ void load_x(float (&x)[4], const AflTfTrainArgs& a, int cid, const Walk& w, int lane,
                                       int wave) {
  // (lane / wave opaque: the row index and the 64-bit column term of the row address are rebuilt here, in the hand-off
  // window where the wave only waits, instead of being held across the step — as loop-invariant state they were the
  // values the one-class allocation spilled to scratch and reloaded inside the step loop)
  asm volatile("" : "+v"(lane));
  asm volatile("" : "+s"(wave));
  const int r = 16 * (wave & 7) + (lane & 15), g = (lane & 63) >> 4;
  const int Bn = min(a.batch, a.nd[cid] - w.b0);
  const gi32* ord = (const gi32*)(a.order + ((long)cid * a.E + w.e) * a.maxnd);
  const bool valid = r < Bn;
  const int ridx = valid ? ord[w.b0 + r] : 0;
  const gf* row = (const gf*)a.rows + (long)ridx * ROW + BrK<BR>::xoff;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = 4 * g + i;
    x[i] = (valid && c < BrK<BR>::din) ? row[c] : 0.f;
  }
}

template <int BR>
__device__ __forceinline__ void branch_main(const AflTfTrainArgs& a, int cid, uchar* smem) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 4;
  float* P = a.params + (long)cid * NPARAM;
  uchar* ws = (uchar*)(a.ws + (long)cid * a.ws_stride);
  gu32* sync = (gu32*)(a.sync + (long)cid * AFL_TF2H_SYNC_WORDS);
  const __amdgpu_buffer_rsrc_t rg = gr_rsrc(sync);  // granule hand-off slots
  for (int i = tid; i < SMEM / 4; i += NTH) ldsf(smem, 0)[i] = 0.f;
  __syncthreads();
  BrState st;
  const __amdgpu_buffer_rsrc_t rm = rsrc(ws + WS_MOM + MOM_WG_BYTES + BR * BR_WG_BYTES);  // this workgroup's units
  br_init<BR>(smem, st, P, rm, lane, wave, tid);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the units' first loads come from other waves' stores)
  __syncthreads();
  Stamp stp;
  stamp_init(stp, a, smem);

  const int nd = a.nd[cid], BS = a.batch, E = a.E;
  const uint32_t seed = a.seeds[cid];
  LDS_AS uint32_t* abort_w = ldsu(smem, B_MISC);
  int step = 0;
  bool failed = false;
  Walk w{0, 0};
  float xin[4];
  bool more = walk_valid(w, nd, BS, E);
  if (more) load_x<BR>(xin, a, cid, w, lane, wave);
  float mka0, mka1;  // the next forward's dropout masks (br_masks), parked through awu / aru
  {
    uint32_t m0, m1;
    br_masks<BR>(afl_hash32(seed, 1u), 16 * wave + (lane & 15), g, m0, m1);
    mka0 = awu(m0);
    mka1 = awu(m1);
  }
  while (more) {
    ++step;
    const AdamK K = adam_k(a, step);
    Saved sv;
    u32x4 outp[2];
    prio_hi();
    asm volatile(";MARK fwd");
    br_forward<BR>(smem, xin, aru(mka0), aru(mka1), sv, outp, lane, wave);
    asm volatile(";MARK fwd_end");
    stp(0, tid);
    gr_put_s(rg, gr_soff(0, BR, wave), 16 * lane, outp, (uint32_t)step);  // this wave's output rows -> head
    prio_lo();
    w.b0 += BS;  // prefetch the next batch's inputs while the head works
    more = walk_valid(w, nd, BS, E);
    if (more) load_x<BR>(xin, a, cid, w, lane, wave);
    {  // the next step's dropout masks, while the head works (this wave would only spin)
      uint32_t m0, m1;
      br_masks<BR>(afl_hash32(seed, (uint32_t)(step + 1)), 16 * wave + (lane & 15), g, m0, m1);
      mka0 = awu(m0);
      mka1 = awu(m1);
    }
    BwdPre bp;  // (while the head works too: the backward then starts on d(out) at once)
    sb();
    br_bwd_pre(smem, sv, bp, lane);
    sb();
    stp(1, tid);
    u32x4 du[2];
    const int go[1] = {gr_soff(1, BR, wave)};
    const uint32_t fv = gr_get_s<1>(rg, go, 16 * lane, du, (uint32_t)step, 1, sync + XF_TMO, lane);  // d(out) of this wave's rows
    prio_hi();  // (the leaders' backward below the laggards' measured -0.5 %: profiles/ab_tf2_r6_update.log)
    stp(2, tid);
    if (fv == 0xFFFFFFFFu) {  // timed out: abort the step for every wave (they wait on this wave's progress)
      if (lane == 0) abort_w[wave] = 1u;
      lds_signal(smem, B_CNT_C, lane);
      lds_signal(smem, B_CNT_A, lane);
      lds_signal(smem, B_CNT_B, lane);
      failed = true;
      break;
    }
    float dout[16];
    unpack16(du, dout);
    if (lane == 0) abort_w[wave] = fv & 1u;
    asm volatile(";MARK bwd");
    br_backward<BR>(smem, dout, sv, bp, K, lane, wave);
    asm volatile(";MARK bwd_end");
    stp(3, tid);
    asm volatile(";MARK upd");
    // (false: the head saw a NaN loss somewhere in the batch — the client's round fails and this step's update is
    // not applied — or a wave stopped making progress)
    const bool upd_ok = br_update<BR>(smem, st, K, lane, wave, tid, step, rm, stp, sync + XF_TMO);
    asm volatile(";MARK upd_end");
    if (!upd_ok) {
      failed = true;
      break;
    }
    stp(5, tid);
    lds_bar();
    stp(6, tid);
  }
  (void)failed;
  stamp_fini(stp, a, smem, tid);
  br_fini<BR>(st, P, rm, lane, wave, tid);
}

// ================================================================================= head workgroup
constexpr Mat HW1{FC1_W, 64, 128, H_IMG_W1, HLD1};
constexpr Mat HW2{FC2_W, 32, 64, H_IMG_W2, HLD2};
__device__ __forceinline__ int hvec_param(int e) {
  return e < 64 ? FC1_B + e : e < 96 ? FC2_B + (e - 64) : e < 128 ? OUT_W + (e - 96) : e == 128 ? OUT_B : -1;
}
struct HdState {
  TS blk[4];  // fc1: k tiles 2(w&3)+{0,1} x n tiles 2(w>>2)+{0,1}
  TS t2;      // fc2: k tile w&3, n tile w>>2
  VS vec;
};

// The head runs as TWO workgroups, halves H0 (batch rows 0-63) and H1 (rows 64-127), so that every wave of the
// step's critical section (hand-off in, forward, loss flags, backward, hand-off out) has a SIMD to itself: in one
// workgroup the head waves w and w + 4 shared a SIMD, and the branch laggards (waves 4-7, the step's critical path)
// were served by the younger head wave of each pair (profiles/ab_tf2_twin_head.log).
//   * Hardware waves 0-3 of a half are its CRITICAL waves: wave c serves row tile 4 half + c — the 16 rows of branch
//     wave 4 half + c — exactly as a head wave of the single workgroup did.
//   * After its d(cat) hand-off a critical wave EXPORTS what the other half needs to hold the full 128-row state:
//     the bf16 cat / a1 / dz1 / dz2 rows (the words it stores into its own LDS tiles), its fp32 column-sum partials
//     and its loss partial, the NaN flag on the tag — EX_SLOTS granule slots (gr_put) per tile and step parity.
//   * Hardware waves 4-7 are the IMPORTERS: wave 4 + c fetches row tile 4 (1 - half) + c of the partner and writes
//     it into this half's LDS tiles, H_PART and H_LOSS at the partner's row / wave positions.  They wait on an LDS
//     counter that their own half's critical waves signal after the d(cat) hand-off, so they issue nothing beside
//     the critical section.
//   * From the loss barrier on both halves run the single workgroup's code on all 8 waves — same tile ownership, same
//     K order, same fixed-order partial sums, same Adam — on bit-identical inputs, so both hold bit-identical weights
//     and nothing is sent back.  H1 has its own moment slab; only H0 writes losses, ok and the parameters.
// Export slots are double-buffered by step parity.  Why export n + 2 cannot overwrite a slot before the partner's
// import n has read it: export n + 2 follows this half's gr_get of the branches' step n + 2 outputs; those follow the
// branches' update n + 1, whose counters need every branch wave's d(out) n + 1, i.e. the d(cat) hand-off of BOTH
// halves' critical waves of step n + 1; the partner's critical waves start step n + 1 after the partner's
// end-of-step-n barrier, which its importers reach only after import n.  (Single slots would race: export n + 1
// needs only the partner's d(cat) n, which precedes its import n.)  Nothing rests on timing or placement; every wait
// is bounded and raises XF_TMO.  A NaN flag reaches both halves (own rows: lossw, partner rows: the export tag) and
// both branches (the d(cat) tag), so all four workgroups leave at the same step.
constexpr int NWG = 4;       // workgroups per client: head halves H0, H1, vitals branch, labs branch
constexpr int EX_SLOTS = 5;  // cat 2, a1 + dz1 2, {dz2, partials, loss} 1
constexpr int EX_BASE = 2 * GR_DIR_BYTES;
static_assert(EX_BASE == AFL_GR_WORDS * 4 && 2 * 8 * EX_SLOTS * 1024 == AFL_EX_WORDS, "export slots follow the hand-off slots");
__device__ __forceinline__ int ex_off(int parity, int tile, int k, int lane) {
  return EX_BASE + ((parity * 8 + tile) * EX_SLOTS + k) * 4096 + lane * 16;
}

__device__ __forceinline__ void head_main(const AflTfTrainArgs& a, int cid, uchar* smem, int half) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 4;
  const bool crit = wave < 4;
  // the row tile this wave serves (critical) or imports (importer), and this lane's batch row
  const int tile = crit ? 4 * half + wave : 4 * (1 - half) + (wave - 4);
  const int r = 16 * tile + (lane & 15);
  float* P = a.params + (long)cid * NPARAM;
  uchar* ws = (uchar*)(a.ws + (long)cid * a.ws_stride);
  gu32* sync = (gu32*)(a.sync + (long)cid * AFL_TF2H_SYNC_WORDS);
  const __amdgpu_buffer_rsrc_t rg = gr_rsrc(sync);  // granule hand-off slots
  for (int i = tid; i < SMEM / 4; i += NTH) ldsf(smem, 0)[i] = 0.f;
  __syncthreads();
  HdState st;
  Stamp stp;
  const __amdgpu_buffer_rsrc_t rm = rsrc(ws + (half == 0 ? WS_MOM : WS_MOM2));  // this workgroup's Adam moments
  mom_zero(rm, tid);
  {
    const int Ta = 2 * (wave & 3), Tb = 2 * (wave >> 2);
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y) tile_load(st.blk[2 * x + y], HW1, Ta + x, Tb + y, lane, P, smem);
    tile_load(st.t2, HW2, wave & 3, wave >> 2, lane, P, smem);
    float p0 = 0.f;
    if (tid < H_NVEC) {
      const int pi = hvec_param(tid);
      p0 = pi >= 0 ? P[pi] : 0.f;
      ldsf(smem, H_VEC)[tid] = p0;
    }
    st.vec = VS{aw(p0)};
  }
  __syncthreads();
  stamp_init(stp, a, smem);

  const int nd = a.nd[cid], BS = a.batch, E = a.E;
  const int nb_total = (nd + BS - 1) / BS;
  const uint32_t seed = a.seeds[cid];
  const uchar* vec = smem + H_VEC;
  LDS_AS float* lossw = ldsf(smem, H_LOSS);
  int step = 0;
  bool failed = false, timed_out = false;
  float epoch_loss = 0.f;
  Walk w{0, 0};
  int cur_e = 0;
  bool more = walk_valid(w, nd, BS, E);
  float lab = 0.f;
  auto load_lab = [&](const Walk& ww) {
    const int Bn = min(BS, nd - ww.b0);
    const gi32* ord = (const gi32*)(a.order + ((long)cid * E + ww.e) * a.maxnd);
    lab = r < Bn ? ((const gf*)a.rows)[(long)ord[ww.b0 + r] * ROW + ROW - 1] : 0.f;
  };
  if (more) load_lab(w);
  while (more) {
    // epoch boundaries crossed since the previous step (skipped batches included) close epoch losses
    while (cur_e < w.e) {
      if (tid == 0 && half == 0) a.losses[(long)cid * E + cur_e] = epoch_loss / (float)max(nb_total, 1);
      epoch_loss = 0.f;
      ++cur_e;
    }
    ++step;
    const AdamK K = adam_k(a, step);
    const int Bn = min(BS, nd - w.b0);
    // the tile's rows as the words its LDS tiles take (bf16 pairs), its loss partial and NaN flag: computed by the
    // tile's critical wave, fetched from the partner's export by its importer
    u32x4 cv[4];  // vitals rows (cv[0..1]) | labs rows (cv[2..3])
    u32x4 a1w[2], dz1w[2], dz2w;
    float lsum = 0.f;
    uint32_t wave_nan = 0u;
    const int par = step & 1;
    if (crit) {
      const uint32_t key = afl_hash32(seed, (uint32_t)step);
      const bool valid = r < Bn;
      const float inv_bn = 1.f / (float)Bn;  // (before the wait: the division is off the critical path)
      // fc1 dropout mask before the wait (the wave would only spin there)
      const uint32_t mh = mask16(key, L_HEAD, r, g, THR_P03);
      sb();
      // ---- branch outputs of this wave's rows
      const int go[2] = {gr_off(0, 0, tile, lane), gr_off(0, 1, tile, lane)};
      const uint32_t fv = gr_get<2>(rg, go, cv, (uint32_t)step, 0, sync + XF_TMO, lane);
      if (fv == 0xFFFFFFFFu) {
        lds_signal(smem, H_CNT, lane);  // (the importers leave through their own bounded waits)
        timed_out = failed = true;
        break;
      }
      prio_hi();  // (one critical wave per SIMD: the importers beside them sleep on H_CNT)
      stp(10, tid);
      // (the dW operands of this step — cat, a1, dz1, dz2 tiles — and the head's column sums are written
      // only AFTER the d(cat) hand-off below: they are off the branches' critical path)
      // ---- fc1 + GELU + dropout(0.3)
      float a1[16], gk1[16];
      {
        f4v acc[4];
#pragma unroll
        for (int T = 0; T < 4; ++T) {
          acc[T] = Z4;
#pragma unroll
          for (int s = 0; s < 4; ++s)
            acc[T] = mma(wfrag(smem + H_IMG_W1, HLD1, T, s, lane), __builtin_bit_cast(s8v, cv[s]), acc[T]);
        }
        float b1[16];
        vec16(b1, vec + HV_B1 * 4, g);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int i = 0; i < 4; i += 2) {
            const int j = 4 * t + i;
            gf2v gp;
            const gf2v gl = gelu2(gf2v{acc[t][i] + b1[j], acc[t][i + 1] + b1[j + 1]}, gp);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              a1[j + h] = keepf(gl[h] * INV_K03, mh, j + h);
              gk1[j + h] = keepf(gp[h] * INV_K03, mh, j + h);
            }
          }
      }
      // ---- fc2 + GELU, output layer, sigmoid, BCE (log clamped at -100)
      float dz2[8], gw[8];
      float dy3 = 0.f, pl = 0.f;
      {
        const s8v b0 = bfrag(a1, 0), b1 = bfrag(a1, 1);
        f4v acc[2];
#pragma unroll
        for (int T = 0; T < 2; ++T) {
          acc[T] = mma(wfrag(smem + H_IMG_W2, HLD2, T, 0, lane), b0, Z4);
          acc[T] = mma(wfrag(smem + H_IMG_W2, HLD2, T, 1, lane), b1, acc[T]);
        }
        float b2[8], wo[8], g2[8], gp2[8];
        vec8(b2, vec + HV_B2 * 4, g);
        vec8(wo, vec + HV_WO * 4, g);
        float dot = 0.f;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int i = 0; i < 4; i += 2) {
            const int j = 4 * t + i;
            gf2v gp;
            const gf2v gl = gelu2(gf2v{acc[t][i] + b2[j], acc[t][i + 1] + b2[j + 1]}, gp);
            g2[j] = gl[0];
            g2[j + 1] = gl[1];
            gp2[j] = gp[0];
            gp2[j + 1] = gp[1];
            dot += g2[j] * wo[j];
            dot += g2[j + 1] * wo[j + 1];
          }
        const float y3 = fk::rsum4(dot) + *(const LDS_AS float*)(vec + HV_BO * 4);
        const float p = sigmoidf_(y3);
        if (valid) {
          // torch's BCELoss gradient (p - y) / max(p (1 - p), 1e-12) times the sigmoid's p (1 - p), as one factor
          // without a division (1 unless the sigmoid saturates; NaN propagates through the compare's false branch)
          const float pq = p * (1.f - p);
          dy3 = (p - lab) * (pq >= 1e-12f ? 1.f : pq * 1e12f) * inv_bn;
        }
        pl = p;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          dz2[j] = dy3 * wo[j] * gp2[j];
          gw[j] = dy3 * g2[j];
        }
      }
      // the NaN-loss abort rides on the hand-off tag: a row's loss is NaN exactly where its gradient factor dy3 is
      // not finite (p or the label NaN; labels are 0 / 1), so the flag needs no loss on the critical path — the loss
      // VALUE (logs, wave sum) is computed after the hand-off, and the head aborts on the same flags
      wave_nan = __builtin_amdgcn_ballot_w64(!(fabsf(dy3) <= 3.402823466e38f)) != 0 ? 1u : 0u;
      // ---- d a1 = dz2 . W2 -> d z1 = d a1 * drop'(.) * gelu'(z1)
      float dz1[16];
      {
        const s8v bz = bfrag(dz2, 0);
#pragma unroll
        for (int T = 0; T < 4; ++T) {
          const f4v acc = mma(wtfrag<true>(smem + H_IMG_W2, HLD2, T, 0, lane), bz, Z4);
#pragma unroll
          for (int i = 0; i < 4; ++i) dz1[4 * T + i] = acc[i] * gk1[4 * T + i];
        }
      }
      // ---- d cat = dz1 . W1, each half straight to its branch
      {
        const s8v b0 = bfrag(dz1, 0), b1 = bfrag(dz1, 1);
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
          float d[16];
#pragma unroll
          for (int Tl = 0; Tl < 4; ++Tl) {
            const int T = 4 * hb + Tl;
            f4v acc = mma(wtfrag<true>(smem + H_IMG_W1, HLD1, T, 0, lane), b0, Z4);
            acc = mma(wtfrag<true>(smem + H_IMG_W1, HLD1, T, 1, lane), b1, acc);
#pragma unroll
            for (int i = 0; i < 4; ++i) d[4 * Tl + i] = acc[i];
          }
          u32x4 u[2];
          pack16(d, u);
          gr_put(rg, gr_off(1, hb, tile, lane), u, ((uint32_t)step << 1) | wave_nan);  // NaN abort rides on the tag
        }
      }
      prio_lo();
      lds_signal(smem, H_CNT, lane);  // this wave's hand-off is out: the importers may start polling
      // ---- export this tile's rows to the partner half (bf16 pairs, the words the LDS tiles below take)
      pack16(a1, a1w);
      pack16(dz1, dz1w);
      dz2w = u32x4{pk2(dz2[0], dz2[1]), pk2(dz2[2], dz2[3]), pk2(dz2[4], dz2[5]), pk2(dz2[6], dz2[7])};
      const uint32_t xtag = ((uint32_t)step << 1) | wave_nan;
      int xl = lane, xt = tile;  // (the export offsets rebuilt here from opaque indices, not held across the step)
      asm volatile("" : "+v"(xl));
      asm volatile("" : "+s"(xt));
      const int xo = ex_off(par, xt, 0, xl);
      {
        const u32x4 c0[2] = {cv[0], cv[1]}, c1[2] = {cv[2], cv[3]};
        gr_put(rg, xo, c0, xtag);
        gr_put(rg, xo + 4096, c1, xtag);
        gr_put(rg, xo + 2 * 4096, a1w, xtag);
        gr_put(rg, xo + 3 * 4096, dz1w, xtag);
      }
      {  // the tile's loss partial (each row counted once: lane group 0), for the loss barrier
        float lrow = 0.f;
        if (valid) {
          // clamp like torch.clamp: NaN must propagate (fmaxf would swallow it)
          float lg, lg1;
          bce_logs(pl, lg, lg1);
          const float lp = lg < -100.f ? -100.f : lg, l1p = lg1 < -100.f ? -100.f : lg1;
          lrow = -(lab * lp + (1.f - lab) * l1p);
        }
        lsum = wave_sum(xl < 16 ? lrow : 0.f);
      }
      {  // the tile's column sums (read after the loss barrier), then the last export slot
        sb();
        // (the partials' lane addresses from the opaque indices too: held across the step, one of them went to scratch)
        LDS_AS float* pt = ldsf(smem, H_PART) + xt * H_NVEC;
        float sb2, swo, sb1;
        const int f2 = colsum32(dz2, xl, sb2), fo = colsum32(gw, xl, swo);
        if (f2 >= 0) {
          pt[HV_B2 + f2] = sb2;
          pt[HV_WO + fo] = swo;
        }
        const int f1 = colsum64(dz1, xl, sb1);
        pt[HV_B1 + f1] = sb1;
        const float dbo = wave_sum(xl < 16 ? dy3 : 0.f);  // d output.bias
        if (xl == 0) pt[HV_BO] = dbo;
        // (the partials as stored, read back lane-major: entries 129..131 are never written and stay 0)
        const LDS_AS float* pr = pt + xl;
        const float p0 = pr[0], p1 = pr[64], p2 = xl < 4 ? pr[128] : 0.f;
        const u32x4 c4[2] = {dz2w, u32x4{__float_as_uint(p0), __float_as_uint(p1), __float_as_uint(p2), __float_as_uint(lsum)}};
        gr_put(rg, xo + 4 * 4096, c4, xtag);
      }
    } else {
      // ---- importer: the partner half's export of row tile `tile`
      prio_lo();
      if (!lds_wait(smem, H_CNT, 4u * (uint32_t)step)) {
        if (lane == 0) __hip_atomic_store(sync + XF_TMO, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        timed_out = failed = true;
        break;
      }
      stp(10, tid);
      int xl = lane, xt = tile;  // (offsets rebuilt here from opaque indices, not held across the step)
      asm volatile("" : "+v"(xl));
      asm volatile("" : "+s"(xt));
      // (two sweeps, the slots written last first: one sweep of all five holds 120 registers)
      const int xo = ex_off(par, xt, 0, xl);
      const int eb[2] = {xo + 3 * 4096, xo + 4 * 4096};
      u32x4 eu[4];
      const uint32_t fv = gr_get<2>(rg, eb, eu, (uint32_t)step, 1, sync + XF_TMO, lane);
      if (fv == 0xFFFFFFFFu) {
        timed_out = failed = true;
        break;
      }
      dz1w[0] = eu[0];
      dz1w[1] = eu[1];
      dz2w = eu[2];
      LDS_AS float* pw = ldsf(smem, H_PART) + xt * H_NVEC + xl;
      pw[0] = __uint_as_float(eu[3][0]);
      pw[64] = __uint_as_float(eu[3][1]);
      if (xl < 4) pw[128] = __uint_as_float(eu[3][2]);
      lsum = __uint_as_float(eu[3][3]);
      wave_nan = fv & 1u;
      const int ea[3] = {xo, xo + 4096, xo + 2 * 4096};
      u32x4 ev[6];
      if (gr_get<3>(rg, ea, ev, (uint32_t)step, 1, sync + XF_TMO, lane) == 0xFFFFFFFFu) {
        timed_out = failed = true;
        break;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) cv[k] = ev[k];
      a1w[0] = ev[4];
      a1w[1] = ev[5];
    }
    // ---- the tile's loss partial and abort flag, and its dW operand rows (read after the loss barrier)
    {
      sb();
      int sl = lane, stl = tile;  // (the tile addresses rebuilt here from opaque indices, not held across the step)
      asm volatile("" : "+v"(sl));
      asm volatile("" : "+s"(stl));
      const int r = 16 * stl + (sl & 15), g = sl >> 4;
      if (sl == 0) {
        lossw[stl] = lsum;
        lossw[8 + stl] = __uint_as_float(wave_nan);
      }
#pragma unroll
      for (int t = 0; t < 8; ++t) {  // cat: tile t of the 8 = half (t & 1) of cv[t >> 1]
        const u32x4 u = cv[t >> 1];
        const u32x2v v = (t & 1) ? u32x2v{u[2], u[3]} : u32x2v{u[0], u[1]};
        *(LDS_AS u32x2v*)(smem + H_CAT + t128(r, 4 * t + g)) = v;
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {  // (words 2t, 2t + 1 of a row: what st4 packs from features 4t .. 4t + 3)
        const int q = 2 * (t & 1);
        *(LDS_AS u32x2v*)(smem + H_A1 + t64(r, 4 * t + g)) = u32x2v{a1w[t >> 1][q], a1w[t >> 1][q + 1]};
        *(LDS_AS u32x2v*)(smem + H_DZ1 + t64(r, 4 * t + g)) = u32x2v{dz1w[t >> 1][q], dz1w[t >> 1][q + 1]};
      }
#pragma unroll
      for (int t = 0; t < 2; ++t) *(LDS_AS u32x2v*)(smem + H_DZ2 + t32(r, 4 * t + g)) = u32x2v{dz2w[2 * t], dz2w[2 * t + 1]};
    }
    stp(11, tid);
    // Adam moments of this step's update (after the hand-off drain, before the loss barrier)
    f4v hm[6], hv[6];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      hm[k] = mom_ld(rm, k, tid);
      hv[k] = mom_ld(rm, 4 + k, tid);
    }
    hm[4] = mom_ld(rm, 8, tid);
    hv[4] = mom_ld(rm, 9, tid);
    hm[5] = mom_ld(rm, 10, tid);
    // the next step's labels (after the hand-off stores: their drain above must not wait for these)
    Walk wn = w;
    wn.b0 += BS;
    more = walk_valid(wn, nd, BS, E);
    lds_bar();
    {
      float tot = 0.f;
      uint32_t any = 0;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        tot += lossw[i];
        any |= __float_as_uint(lossw[8 + i]);
      }
      const float loss = tot / (float)Bn;
      if (any) {  // a NaN loss (uniform across the workgroup; the branches abort on the same per-wave flags)
        failed = true;
        break;
      }
      epoch_loss += loss;
    }
    if (more) load_lab(wn);
    w = wn;
    stp(12, tid);
    // ---- weight gradients + Adam
    {
      int ln = lane, wv = wave;
      opq(ln, wv);  // (the phase's tile addresses recomputed here, not held across the step)
      const int Ta = 2 * (wv & 3), Tb = 2 * (wv >> 2);
      f4v acc[2][2] = {{Z4, Z4}, {Z4, Z4}};
      f4v a2 = Z4;
      const int T2 = wv & 3, Tn2 = wv >> 2;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const s8v x0 = tfrag<TK128>(smem + H_CAT, 32 * s, Ta, ln), x1 = tfrag<TK128>(smem + H_CAT, 32 * s, Ta + 1, ln);
        const s8v y0 = tfrag<TK64>(smem + H_DZ1, 32 * s, Tb, ln), y1 = tfrag<TK64>(smem + H_DZ1, 32 * s, Tb + 1, ln);
        acc[0][0] = mma(x0, y0, acc[0][0]);
        acc[0][1] = mma(x0, y1, acc[0][1]);
        acc[1][0] = mma(x1, y0, acc[1][0]);
        acc[1][1] = mma(x1, y1, acc[1][1]);
        a2 = mma(tfrag<TK64>(smem + H_A1, 32 * s, T2, ln), tfrag<TK32>(smem + H_DZ2, 32 * s, Tn2, ln), a2);
      }
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
          if (!ABL(K, ABL_HEADUPD))
            tile_adam(st.blk[2 * x + y], hm[2 * x + y], hv[2 * x + y], HW1, Ta + x, Tb + y, ln, acc[x][y], K, smem);
      if (!ABL(K, ABL_HEADUPD)) tile_adam(st.t2, hm[4], hv[4], HW2, T2, Tn2, ln, a2, K, smem);
      if (tid < H_NVEC) {
        // the 8 waves' partial sums in a fixed order: bit-reproducible whatever order the waves ran in
        // (one lane address, rebuilt here, for the partials and the entry: H_PART follows H_VEC; held across the step
        // as two hoisted addresses, one of them went to scratch)
        int t = tid;
        asm volatile("" : "+v"(t));
        LDS_AS float* ve = ldsf(smem, H_VEC) + t;
        const LDS_AS float* c = ve + H_NVEC;
        static_assert(H_PART == H_VEC + H_NVEC * 4, "the partial sums follow the vector");
        float gsum = c[0];
#pragma unroll
        for (int w8 = 1; w8 < 8; ++w8) gsum += c[w8 * H_NVEC];
        float vm = hm[5][0], vvv = hm[5][1];
        if (hvec_param(tid) >= 0) *ve = adam1(st.vec.p, vm, vvv, gsum, K);
        hm[5][0] = vm;
        hm[5][1] = vvv;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        mom_st(rm, k, tid, hm[k]);
        mom_st(rm, 4 + k, tid, hv[k]);
      }
      mom_st(rm, 8, tid, hm[4]);
      mom_st(rm, 9, tid, hv[4]);
      mom_st(rm, 10, tid, hm[5]);
    }
    stp(13, tid);
    lds_bar();
    stp(14, tid);
  }
  stamp_fini(stp, a, smem, tid);
  if (!failed) {
    while (cur_e < E) {  // the last epoch (and trailing epochs that had no step)
      if (tid == 0 && half == 0) a.losses[(long)cid * E + cur_e] = epoch_loss / (float)max(nb_total, 1);
      epoch_loss = 0.f;
      ++cur_e;
    }
  }
  // parameters back, from H0 (H1 holds the same bits; a failed client keeps its pre-step values: the failing step
  // applied no update)
  if (half != 0) return;
  {
    int ln = lane, wv = wave;
    opq(ln, wv);  // (addresses recomputed here, not carried from the prologue's tile loads across the step loop)
    const int Ta = 2 * (wv & 3), Tb = 2 * (wv >> 2);
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y) tile_store(st.blk[2 * x + y], HW1, Ta + x, Tb + y, ln, P);
    tile_store(st.t2, HW2, wv & 3, wv >> 2, ln, P);
    if (tid < H_NVEC && hvec_param(tid) >= 0) P[hvec_param(tid)] = ar(st.vec.p);
  }
  if (tid == 0) {
    const bool tmo = timed_out || __hip_atomic_load(sync + XF_TMO, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    a.ok[cid] = tmo ? -1 : (failed ? 0 : 1);
  }
}

}  // namespace t2

#ifdef TF2_STAMPS
#define K_TF2 k_tf2_train_stamped
#else
#define K_TF2 k_tf2_train
#endif
// 4 workgroups per client: blocks c (head half H0), CP + c (head half H1), 2 CP + c (vitals branch), 3 CP + c (labs
// branch).  Role-major block order
// with a block stride CP padded to a multiple of 8 when the grid still fits: a client's workgroups are blocks
// role * CP + cid, which the round-robin dispatch deals to ONE XCD (same-L2 hand-offs; speed only, never
// correctness); padding blocks (cid >= C) exit at once.
__global__ void __launch_bounds__(t2::NTH) K_TF2(AflTfTrainArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int cp = a.cpad > 0 ? a.cpad : a.C;
  const int role = blockIdx.x / cp, cid = blockIdx.x - role * cp;
  if (cid >= a.C) return;
#if defined(TF2_ROLE)
  if (TF2_ROLE < 2) t2::head_main(a, cid, smem, TF2_ROLE);
  else if (TF2_ROLE == 2) t2::branch_main<0>(a, cid, smem);
  else t2::branch_main<1>(a, cid, smem);
  (void)role;
#else
  if (role < 2)
    t2::head_main(a, cid, smem, role);
  else if (role == 2)
    t2::branch_main<0>(a, cid, smem);
  else
    t2::branch_main<1>(a, cid, smem);
#endif
}

#ifndef TF2_STAMPS
// Determinism check of the cross-wave column-sum accumulator (onchip.h lds_addq), used by the tests: W waves
// each add their 64 partials (vals [W][64]) into 64 slots after a per-wave delay drawn from `seed` (so the
// arrival order changes from launch to launch); out [64] = the decoded sums.  mode 1: the unquantised fp64 LDS
// atomics the trainers used before (order-dependent once the partials span more than ~2^29).
__global__ void __launch_bounds__(1024) k_fxsum_test(const float* __restrict__ vals, int W, uint32_t seed, int mode,
                                                   float* __restrict__ out) {
  __shared__ double q[64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (threadIdx.x < 64) q[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t spins = afl_hash32(seed, (uint32_t)w) & 1023u;
  for (uint32_t i = 0; i < spins; ++i) __builtin_amdgcn_s_sleep(1);
  const float v = vals[w * 64 + lane];
  if (mode == 0)
    oc::lds_addq((oc::uchar*)q, lane, v);
  else
    __hip_atomic_fetch_add((LDS_AS double*)q + lane, (double)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __syncthreads();
  if (threadIdx.x < 64)
    out[lane] = mode == 0 ? oc::lds_getq((const oc::uchar*)q, lane)
                          : (float)((LDS_AS double*)q)[lane];
}
int afl_fxsum_test(const float* vals, int W, uint32_t seed, int mode, float* out, hipStream_t s) {
  if (W < 1 || W > 8) return -1;  // (at most 8 partials per slot: onchip.h lds_addq)
  hipLaunchKernelGGL(k_fxsum_test, dim3(1), dim3(64 * W), 0, s, vals, W, seed, mode, out);
  return (int)hipGetLastError();
}
#endif

#ifdef TF2_STAMPS
int afl_tf2_train_stamped(const AflTfTrainArgs* a, hipStream_t s) {
#else
long afl_tf2_ws_floats() { return t2::WS_BYTES / 4; }
int afl_tf2_wgs_per_client() { return t2::NWG; }

int afl_tf2_train(const AflTfTrainArgs* a, hipStream_t s) {
  if (a->stamps) return afl_tf2_train_stamped(a, s);
#endif
  const int wgs = t2::NWG;
  int cus = 0;
  if (const int rc = afl_launch_preamble(a, 2, 128, true, true, (const void*)K_TF2, t2::SMEM, wgs, &cus)) return rc;
  AflTfTrainArgs b = *a;
  b.cpad = (a->C + 7) / 8 * 8;  // (measured neutral against the unpadded grid: profiles/ab_tf2_r5_row_split.log)
  if (wgs * b.cpad > cus) b.cpad = a->C;
  hipLaunchKernelGGL(K_TF2, dim3(wgs * b.cpad), dim3(t2::NTH), t2::SMEM, s, b);
  return 0;
}
