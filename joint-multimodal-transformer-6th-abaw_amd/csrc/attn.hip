// Fused scaled-dot-product attention for the JMT path (gfx950, wave64), head_dim 512, per
// (batch n, head h):
//   forward:  O = softmax(scale Q K^T) V, + lse (natural log of the row sums, scaled scores)
//   backward: P = exp(scale Q K^T - lse) recomputed, dP = dO V^T, Delta = rowsum(dO o O),
//             dS = scale P o (dP - Delta), dQ = dS K;  P and dS written once (bf16/f16) for the
//             dK = dS^T Q / dV = P^T dO GEMMs
// Replaces the score GEMM -> softmax -> PV GEMM chain behind every nn.MultiheadAttention of the
// reference (F.multi_head_attention_forward, called from mm_multi_transformers.py:57,142-167,
// 191 and intra_modal_transformer_fusion.py) and its autograd backward.
//
// Two geometries.  Whole rows (round 6 backward attn_bwd_pds_kernel, round 7 forward
// attn_fwd_rows_kernel; their own headers below): a block is 8 waves x 16 rows = 128 rows, a wave
// contracts all 512 head dims itself, 32-key tiles double-buffered, one barrier per tile, 128 KiB
// of LDS.  jmt_attn_fwd takes it for Lq > 64 (JMT_ATTN_FWD_ROWS=0: never); Lq <= 64 stays on the
// 64-row kernel, whose arithmetic attn_short.hip reproduces bit for bit.
// Half rows (attn_fwd_kernel, attn_bwd_kernel): a block is 8 waves (512 threads, 2 waves per SIMD
// at one block per CU) owning 64 rows of the row operand (Q forward, Q / dO backward).  Wave w owns rows
// 16 (w & 3) .. +15 and HALF h = w >> 2 of the 512 head dims: its row-operand fragments
// (16 rows x 256 dims) and its accumulator (O or dQ: 16 rows x 256 dims, 64 registers) stay in
// registers.  The contraction over head dims of the score products (Q K^T, dO V^T) is split
// between the two waves of a pair (w, w ^ 4): each writes its 16 x KT fp32 partial into an LDS
// exchange slot, the pair adds them in one canonical order (half 0 + half 1, so both hold
// bitwise the same scores), and both run the same softmax; the update products (P V, dS K)
// need no exchange: each wave produces its own 256 output dims.  This halves the registers of
// the round-1 kernel (453 VGPRs, one wave per SIMD) so two waves per SIMD hide LDS / MFMA
// latency.
//
//  * MFMA operands swapped (stream operand first): an accumulator lane owns ONE row and 4
//    consecutive keys / dims, softmax row state is lane-local (2 shuffles per row reduction),
//    probabilities (or dS) feed the update MFMA straight from registers (their k-slot order is
//    mirrored in the transposed fragment reads of the stream image).
//  * K / V images: [rows][1024 B] with no padding, 16-B chunk c of row r stored at chunk
//    c ^ ((r & 7) << 1): the ds_read_b128 score fragments and the ds_read_b64_tr_b16 update
//    fragments are both conflict-free.  Filled by LDS-DMA (one 1-KiB wave-instruction per row,
//    the swizzle applied to the per-lane SOURCE address, the LDS side linear).
//  * Forward: 64-key tiles, K and V in one image each (K of tile j+1 lands during the P V of
//    tile j, V of tile j+1 during the scores of tile j+1); online softmax with LAZY rescaling
//    (the reference max is raised only when a row max exceeds it by > 8 in log2 units).
//    LDS: K 64 KiB + V 64 KiB + exchange 32 KiB = 160 KiB.
//  * Backward: 32-key tiles double-buffered (tile j+1's K and V land during tile j), scores and
//    dP exchanged together.  LDS: 2 x (K 32 KiB + V 32 KiB) + exchange 32 KiB = 160 KiB.
//  * Persistent grid (one block per CU, item_range): an item = (n, h, 64-row q-tile); the next
//    item's row fragments and K / V tile 0 are issued during the current item's last tile, and
//    the outputs (O, dQ) are stored straight from registers (16-B stores of paired accumulators),
//    so consecutive items overlap their loads and stores (3-7 % over one block per item).
//  * Waits: raw s_barrier after an explicit lgkmcnt(0); LDS-DMA retired by vmcnt before the
//    barrier that precedes the read (never __syncthreads, whose fence would drain the DMA).
//  * XCD-aware item order: the q-tiles of one (n, h) run on one XCD and share K / V in its L2.
#include "attn_common.h"

namespace jmt {

constexpr int AT_QT = 64;           // rows per block
constexpr int AF_KT = 64;           // forward keys per tile
constexpr int AB_KT = 32;           // backward keys per tile
constexpr int AT_XCH = 4096;        // exchange bytes per wave
constexpr int AF_LDS = 2 * AF_KT * AT_ROWB + 8 * AT_XCH;   // 160 KiB
constexpr int AB_LDS = 4 * AB_KT * AT_ROWB + 8 * AT_XCH;   // 160 KiB

struct AttnFwdArgs {
  const void* q;
  const void* k;
  const void* v;
  void* o;
  float* lse;
  int64_t sq_l, sq_n, sk_l, sk_n, sv_l, sv_n, so_l, so_n;
  int Lq, Lk, H, nitems;
  float scale_log2;
  uint64_t* stamps;
  QShare qs;                        // the whole-row kernel only (jmt_attn_fwd_sq)
};

// Phase stamps (diagnostic build only, STAMP = true): s_memtime at each phase boundary of every
// tile of one block in the middle of the grid, stored by every lane of waves 0 and 4 at a
// lane-indexed address (vector stores).
template <bool STAMP>
__device__ __forceinline__ void stamp(uint64_t* buf, int idx) {
  if constexpr (STAMP) {
    if (buf && blockIdx.x == gridDim.x / 2 && ((threadIdx.x >> 6) & 3) == 0) {
      const uint64_t t = __builtin_amdgcn_s_memtime();
      buf[((threadIdx.x >> 8) * 256 + idx) * 64 + (threadIdx.x & 63)] = t;
    }
  }
}

// OPT (compile-time schedule bits, ATTN_FWD_OPT below): 1 lane-group reductions by permlane swaps
// instead of ds_bpermute shuffles; 2 s_setprio(1) for the second-dispatched half (waves 4-7, the
// arbitration loser of every phase: MI355X_MICROARCH "Two waves per SIMD" item 4); 4 the next
// K tile's LDS-DMA issued in pieces between the P V MFMA batches instead of in one burst after
// the score barrier; 8 the exponentials of keys 32-63 issued between the first P V batches
// (which read only keys 0-31), VALU beside the MFMAs.
template <typename T, bool STAMP = false, int OPT = 0>
__global__ __launch_bounds__(512, 2) void attn_fwd_kernel(AttnFwdArgs p) {
  typedef typename Frag16<T>::t F;
  typedef typename Frag16<T>::h Hf;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* kimg = smem;
  char* vimg = smem + AF_KT * AT_ROWB;
  char* xch = smem + 2 * AF_KT * AT_ROWB;

  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int g = lane >> 4, li = lane & 15, rg = w & 3, h = w >> 2;
  const int nqt = (p.Lq + AT_QT - 1) / AT_QT;
  const int nkt = (p.Lk + AF_KT - 1) / AF_KT;
  int item, iend, istride;
  item_range(p.nitems, item, iend, istride);
  if (item >= iend) return;
  if constexpr ((OPT & 2) != 0)
    if (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) >= 4) __builtin_amdgcn_s_setprio(1);

  // item -> (n, head, first query row)
  int nh = item / nqt, n = nh / p.H, hd = nh % p.H, q0 = (item % nqt) * AT_QT;
  const T* kb = (const T*)p.k + (int64_t)n * p.sk_n + hd * AT_DH;
  const T* vb = (const T*)p.v + (int64_t)n * p.sv_n + hd * AT_DH;

  F qf[8];
  auto load_q = [&](int n_, int hd_, int q0_) {
    const T* qrow = (const T*)p.q + (int64_t)n_ * p.sq_n + hd_ * AT_DH +
                    (int64_t)min(q0_ + 16 * rg + li, p.Lq - 1) * p.sq_l + 256 * h + 8 * g;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) qf[ks] = *(const F*)(qrow + 32 * ks);
  };
  load_q(n, hd, q0);
  stage_rows<T, AF_KT, 8, true>(kimg, kb, p.sk_l, 0, p.Lk);
  stage_rows<T, AF_KT, 8, true>(vimg, vb, p.sv_l, 0, p.Lk);

  f32x4* xmine = (f32x4*)(xch + w * AT_XCH) + lane;
  const f32x4* xpart = (const f32x4*)(xch + (w ^ 4) * AT_XCH) + lane;
  int kb4[4], tb8[8];
#pragma unroll
  for (int m = 0; m < 4; ++m) kb4[m] = row_base(m, li, g, h);
#pragma unroll
  for (int c = 0; c < 8; ++c) tb8[c] = tr_base(c, li, g, h);

  // Per item: Q (registers) and K / V tile 0 (LDS) were issued during the previous item's last
  // tile (K tile 0 and Q right after its score phase freed the K image and Q registers, V tile 0
  // after its P V phase), so an item's loads overlap the previous item's softmax, P V and output
  // stores instead of opening every block with a cold load.
  while (true) {
    const int qr = q0 + 16 * rg + li;
    const int nxt = item + istride;
    const bool more = nxt < iend;
    const int nh2 = nxt / nqt, n2 = nh2 / p.H, hd2 = nh2 % p.H, q02 = (nxt % nqt) * AT_QT;
    const T* kb2 = (const T*)p.k + (int64_t)n2 * p.sk_n + hd2 * AT_DH;
    const T* vb2 = (const T*)p.v + (int64_t)n2 * p.sv_n + hd2 * AT_DH;

    f32x4 o[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;

    wait_vmcnt<AF_KT / 8>();                        // Q and K tile 0 landed (V 0 in flight)
    lds_barrier();
    stamp<STAMP>(p.stamps, 255);
    for (int j = 0; j < nkt; ++j) {
      stamp<STAMP>(p.stamps, 8 * j);
      // ---- partial scores over this wave's 256 dims: s[kt][r] = <row qr, key 64j+16kt+4g+r>
      f32x4 s[4];
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
      {   // k-step batches of 4 fragments (key subtiles 0..3), double-buffered: the reads of
          // batch ks+1 are in flight while the 4 MFMAs of batch ks run (pinned by sched_barrier)
        F fa[4], fb[4];
        auto kbatch = [&](F* dst, int ks) {
#pragma unroll
          for (int kt = 0; kt < 4; ++kt)
            dst[kt] = *(const F*)(kimg + kb4[ks & 3] + 256 * (ks >> 2) + 16384 * kt);
        };
        kbatch(fa, 0);
#pragma unroll
        for (int ks = 0; ks < 8; ks += 2) {
          kbatch(fb, ks + 1);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int kt = 0; kt < 4; ++kt) s[kt] = mfma16(fa[kt], qf[ks], s[kt]);
          __builtin_amdgcn_sched_barrier(0);
          if (ks + 2 < 8) kbatch(fa, ks + 2);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int kt = 0; kt < 4; ++kt) s[kt] = mfma16(fb[kt], qf[ks + 1], s[kt]);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      stamp<STAMP>(p.stamps, 8 * j + 1);
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) xmine[64 * kt] = s[kt];
      wait_vmcnt<0>();                              // V tile j landed
      stamp<STAMP>(p.stamps, 8 * j + 2);
      lds_barrier();                                // partials visible; K image free
      stamp<STAMP>(p.stamps, 8 * j + 3);
      // the K image is free: K tile j+1 (or the next item's tile 0) is staged now, or in pieces
      // between the P V batches below (OPT & 4)
      const bool stage_k = j + 1 < nkt || more;
      const T* kb_next = j + 1 < nkt ? kb : kb2;
      const int k0_next = j + 1 < nkt ? AF_KT * (j + 1) : 0;
      if constexpr ((OPT & 4) == 0) {
        if (stage_k) stage_rows<T, AF_KT, 8, true>(kimg, kb_next, p.sk_l, k0_next, p.Lk);
      }
      if (j + 1 == nkt && more) load_q(n2, hd2, q02);   // next item's Q (registers free)
      const int kbase = AF_KT * j + 4 * g;
      float mx = -INFINITY;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        const f32x4 ps = xpart[64 * kt];
        const f32x4 full = h == 0 ? s[kt] + ps : ps + s[kt];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float x = (kbase + 16 * kt + r < p.Lk) ? full[r] * p.scale_log2 : -INFINITY;
          s[kt][r] = x;
          mx = fmaxf(mx, x);
        }
      }
      if constexpr ((OPT & 1) != 0) {
        mx = pl_pair_max(mx);
      } else {
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      }
      if (__any(mx > m_run + 8.f)) {                // lazy rescale (header)
        const float m_new = fmaxf(m_run, mx);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        m_run = m_new;
        l_run *= alpha;
#pragma unroll
        for (int t = 0; t < 16; ++t) o[t] *= alpha;
      }
      F pf[2];
      float ls = 0.f;
      auto exps = [&](int kt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pv = __builtin_amdgcn_exp2f(s[kt][r] - m_run);
          ls += pv;
          pf[kt >> 1][(kt & 1) * 4 + r] = from_f<T>(pv);
        }
      };
      // OPT & 8: the probabilities of keys 32-63 (pf[1]) are exponentiated between the first
      // P V batches, which only read pf[0] (VALU beside the MFMAs); same summation order
      exps(0);
      exps(1);
      if constexpr ((OPT & 8) == 0) {
        exps(2);
        exps(3);
        l_run += ls;
      }
      stamp<STAMP>(p.stamps, 8 * j + 4);
      // ---- o[t] += sum_k P(k) V[k][256h + 16t + 4g + r]: transposed fragment reads of the V
      // image in double-buffered batches of 4 fragments (q = 4b + i: t = q % 16, u = q / 16)
      {
        F fa[4], fb[4];
        auto vbatch = [&](F* dst, int b) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int q = 4 * b + i, u = q >> 4, t = q & 15;
            const char* a = vimg + tb8[t & 7] + 256 * (t >> 3) + 32768 * u;
            const Hf lo = tr_read<Hf>(a);
            const Hf hi = tr_read<Hf>(a + 16384);
            dst[i] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
          }
        };
        vbatch(fa, 0);
#pragma unroll
        for (int b = 0; b < 8; b += 2) {
          vbatch(fb, b + 1);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int q = 4 * b + i;
            o[q & 15] = mfma16(fa[i], pf[q >> 4], o[q & 15]);
          }
          __builtin_amdgcn_sched_barrier(0);
          if constexpr ((OPT & 4) != 0) {           // 2 of the 8 K-tile pieces per batch pair
            constexpr int NP = AF_KT / 8;
            if (stage_k)
              stage_rows_part<T, AF_KT, 8, true>(kimg, kb_next, p.sk_l, k0_next, p.Lk, (b / 2) * NP / 4,
                                        (b / 2 + 1) * NP / 4);
            __builtin_amdgcn_sched_barrier(0);
          }
          if constexpr ((OPT & 8) != 0) {
            if (b < 4) exps(2 + b / 2);             // pf[1] before the batches that read it
            if (b == 2) l_run += ls;
            __builtin_amdgcn_sched_barrier(0);
          }
          if (b + 2 < 8) vbatch(fa, b + 2);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int q = 4 * (b + 1) + i;
            o[q & 15] = mfma16(fb[i], pf[q >> 4], o[q & 15]);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      stamp<STAMP>(p.stamps, 8 * j + 5);
      if (j + 1 < nkt) {
        wait_vmcnt<0>();                            // K tile j+1 landed
        stamp<STAMP>(p.stamps, 8 * j + 6);
        lds_barrier();                              // V image and exchange slots free
        stage_rows<T, AF_KT, 8, true>(vimg, vb, p.sv_l, AF_KT * (j + 1), p.Lk);
      }
    }
    stamp<STAMP>(p.stamps, 254);
    float lt = l_run;
    if constexpr ((OPT & 1) != 0) {
      lt = pl_pair_sum(lt);
    } else {
      lt += __shfl_xor(lt, 16, 64);
      lt += __shfl_xor(lt, 32, 64);
    }
    JMT_DCHECK(item < p.nitems && n * p.H + hd == nh);
    if (qr < p.Lq && g == 0 && h == 0 && p.lse)
      p.lse[(int64_t)nh * p.Lq + qr] = (m_run + __builtin_amdgcn_logf(lt)) * 0.69314718055994531f;
    store_acc_direct<T>(o, 1.f / lt,
                        (T*)p.o + (int64_t)n * p.so_n + hd * AT_DH + (int64_t)qr * p.so_l + 256 * h,
                        qr < p.Lq);
    if (!more) break;
    lds_barrier();                                  // every wave is done with the V image
    stage_rows<T, AF_KT, 8, true>(vimg, vb2, p.sv_l, 0, p.Lk);
    item = nxt; nh = nh2; n = n2; hd = hd2; q0 = q02; kb = kb2; vb = vb2;
  }
}


// (A software-pipelined form — each tile's P V deferred into the next tile's iteration and
// interleaved with its exponentials, the last P V of an item run in the next item's first
// iteration — measured 3-8 % slower than this kernel at N = 96-384: profiles/
// r02_attn_pipelined_fwd.txt.)
// (A 4-wave, one-wave-per-SIMD forward with v_mfma_f32_32x32x16, 32 rows x all 512 dims per wave
// and 128 rows per block — half the K/V bytes into LDS and half the LDS fragment bytes per FLOP —
// needs ~480 registers per wave (O 256 + Q 128 + working set) and spilled 256 VGPRs under hipcc:
// not kept.  Phase stamps of this 16x16 kernel: profiles/r02_attn_phase_stamps.txt.)


// OPT: as attn_fwd_kernel (1 permlane reductions of Delta, 2 s_setprio(1) for waves 4-7, 4 the
// next tile's K / V LDS-DMA issued in pieces between the score / dP MFMA batches); 16 each
// tile's P / dS row stores deferred to the start of the next tile: the end-of-tile
// vmcnt(0) that waits for the next tile's DMA otherwise also waits for the acknowledgement of
// the stores issued just before it (stores count in vmcnt, in issue order)
template <typename T, int OPT = 0>
__global__ __launch_bounds__(512, 2) void attn_bwd_kernel(AttnBwdArgs p) {
  typedef typename Frag16<T>::t F;
  typedef typename Frag16<T>::h Hf;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int IMG = AB_KT * AT_ROWB;            // one K or V image
  char* xch = smem + 4 * IMG;

  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int g = lane >> 4, li = lane & 15, rg = w & 3, h = w >> 2;
  const int nqt = (p.Lq + AT_QT - 1) / AT_QT;
  const int nkt = (p.Lk + AB_KT - 1) / AB_KT;
  int item, iend, istride;
  item_range(p.nitems, item, iend, istride);
  if (item >= iend) return;
  if constexpr ((OPT & 2) != 0)
    if (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) >= 4) __builtin_amdgcn_s_setprio(1);

  int nh = item / nqt, n = nh / p.H, hd = nh % p.H, q0 = (item % nqt) * AT_QT;
  const T* kb = (const T*)p.k + (int64_t)n * p.sk_n + hd * AT_DH;
  const T* vb = (const T*)p.v + (int64_t)n * p.sv_n + hd * AT_DH;

  // row-operand fragments of an item: Q, dO (kept for the whole item) and O (Delta only)
  F qf[8], df[8], of[8];
  auto rows_off = [&](int q0_) { return (int64_t)min(q0_ + 16 * rg + li, p.Lq - 1); };
  auto load_qd = [&](int n_, int hd_, int q0_) {
    const int64_t qc_ = rows_off(q0_), coff = (int64_t)hd_ * AT_DH + 256 * h + 8 * g;
    const T* qrow = (const T*)p.q + (int64_t)n_ * p.sq_n + qc_ * p.sq_l + coff;
    const T* drow = (const T*)p.go + (int64_t)n_ * p.sgo_n + qc_ * p.sgo_l + coff;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      qf[ks] = *(const F*)(qrow + 32 * ks);
      df[ks] = *(const F*)(drow + 32 * ks);
    }
  };
  auto load_o = [&](int n_, int hd_, int q0_) {
    const int64_t qc_ = rows_off(q0_), coff = (int64_t)hd_ * AT_DH + 256 * h + 8 * g;
    const T* orow = (const T*)p.o + (int64_t)n_ * p.so_n + qc_ * p.so_l + coff;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) of[ks] = *(const F*)(orow + 32 * ks);
  };
  load_qd(n, hd, q0);
  load_o(n, hd, q0);
  int buf = 0;                                    // buffer pair of the next tile to compute
  stage_rows<T, AB_KT>(smem, kb, p.sk_l, 0, p.Lk);
  stage_rows<T, AB_KT>(smem + IMG, vb, p.sv_l, 0, p.Lk);

  f32x4* xmine = (f32x4*)(xch + w * AT_XCH) + lane;
  const f32x4* xpart = (const f32x4*)(xch + (w ^ 4) * AT_XCH) + lane;
  int kb4[4], tb8[8];
#pragma unroll
  for (int m = 0; m < 4; ++m) kb4[m] = row_base(m, li, g, h);
#pragma unroll
  for (int c = 0; c < 8; ++c) tb8[c] = tr_base(c, li, g, h);

  // Persistent items (item_range): the next item's Q / dO / O fragments are loaded right after
  // the last tile's score phase (their registers are free from there on) and its K / V tile 0
  // into the free buffer pair at the start of the last tile, so an item opens on landed data.
  while (true) {
    const int qr = q0 + 16 * rg + li;
    const int qc = min(qr, p.Lq - 1);
    const int64_t prow = (int64_t)nh * p.Lq + qc;
    const int nxt = item + istride;
    const bool more = nxt < iend;
    const int nh2 = nxt / nqt, n2 = nh2 / p.H, hd2 = nh2 % p.H, q02 = (nxt % nqt) * AT_QT;
    const T* kb2 = (const T*)p.k + (int64_t)n2 * p.sk_n + hd2 * AT_DH;
    const T* vb2 = (const T*)p.v + (int64_t)n2 * p.sv_n + hd2 * AT_DH;

    float delta;
    {
      float dp = 0.f;
#pragma unroll
      for (int ks = 0; ks < 8; ++ks)
#pragma unroll
        for (int e = 0; e < 8; ++e) dp += (float)of[ks][e] * (float)df[ks][e];
      if constexpr ((OPT & 1) != 0) {
        dp = pl_pair_sum(dp);
      } else {
        dp += __shfl_xor(dp, 16, 64);
        dp += __shfl_xor(dp, 32, 64);
      }
      delta = dp;                                   // this half's part of rowsum(dO o O)
    }
    const float lse2 = p.lse[prow] * 1.4426950408889634f;
    ((float*)xch)[w * 64 + lane] = delta;

    f32x4 acc[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    T* prow_p = (T*)p.pbuf + prow * p.ldp;
    T* prow_ds = (T*)p.dsbuf + prow * p.ldp;

    wait_vmcnt<0>();                                // tile 0 landed
    lds_barrier();                                  // ... and every Delta part written
    {
      const float part = ((const float*)xch)[(w ^ 4) * 64 + lane];
      delta = h == 0 ? delta + part : part + delta;
    }
    lds_barrier();                                  // Delta parts read: exchange slots free

    uint2 pend[2];                                  // OPT & 16: the previous tile's P / dS
    int pend_key[2] = {0, 0};
    bool pend_on = false;
    auto flush = [&]() {
      if (pend_on) {
        T* rowp = h == 0 ? prow_p : prow_ds;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
          if (qr < p.Lq && pend_key[kt] < p.ldp) *(uint2*)(rowp + pend_key[kt]) = pend[kt];
        pend_on = false;
      }
    };
    for (int j = 0; j < nkt; ++j) {
      const char* kimg = smem + buf * 2 * IMG;
      const char* vimg = kimg + IMG;
      if constexpr ((OPT & 16) != 0) flush();       // older than this tile's DMA
      char* nk = smem + (buf ^ 1) * 2 * IMG;        // tile j+1 (or the next item's tile 0)
      const bool stage_n = j + 1 < nkt || more;
      const T* kbn = j + 1 < nkt ? kb : kb2;
      const T* vbn = j + 1 < nkt ? vb : vb2;
      const int k0n = j + 1 < nkt ? AB_KT * (j + 1) : 0;
      if constexpr ((OPT & 4) == 0) {
        if (stage_n) {
          stage_rows<T, AB_KT>(nk, kbn, p.sk_l, k0n, p.Lk);
          stage_rows<T, AB_KT>(nk + IMG, vbn, p.sv_l, k0n, p.Lk);
        }
      }
      // ---- partial scores (K) and partial dP (V) over this wave's 256 dims
      f32x4 s[2], d[2];
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
        d[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      {   // k-step batches (K and V fragments of key subtiles 0, 1), double-buffered
        F fa[4], fb[4];
        auto batch = [&](F* dst, int ks) {
#pragma unroll
          for (int kt = 0; kt < 2; ++kt) {
            const int o = kb4[ks & 3] + 256 * (ks >> 2) + 16384 * kt;
            dst[kt] = *(const F*)(kimg + o);
            dst[2 + kt] = *(const F*)(vimg + o);
          }
        };
        batch(fa, 0);
#pragma unroll
        for (int ks = 0; ks < 8; ks += 2) {
          batch(fb, ks + 1);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int kt = 0; kt < 2; ++kt) {
            s[kt] = mfma16(fa[kt], qf[ks], s[kt]);
            d[kt] = mfma16(fa[2 + kt], df[ks], d[kt]);
          }
          __builtin_amdgcn_sched_barrier(0);
          if (ks + 2 < 8) batch(fa, ks + 2);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int kt = 0; kt < 2; ++kt) {
            s[kt] = mfma16(fb[kt], qf[ks + 1], s[kt]);
            d[kt] = mfma16(fb[2 + kt], df[ks + 1], d[kt]);
          }
          __builtin_amdgcn_sched_barrier(0);
          if constexpr ((OPT & 4) != 0) {           // K then V pieces, 2 per batch pair
            constexpr int NP = AB_KT / 8;           // pieces per image per wave (4)
            if (stage_n) {
              if (ks < 4)
                stage_rows_part<T, AB_KT>(nk, kbn, p.sk_l, k0n, p.Lk, (ks / 2) * NP / 2,
                                          (ks / 2 + 1) * NP / 2);
              else
                stage_rows_part<T, AB_KT>(nk + IMG, vbn, p.sv_l, k0n, p.Lk,
                                          (ks / 2 - 2) * NP / 2, (ks / 2 - 1) * NP / 2);
            }
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
      xmine[0] = s[0];
      xmine[64] = s[1];
      xmine[128] = d[0];
      xmine[192] = d[1];
      lds_barrier();                                // partials visible (tile j+1 DMA in flight)
      if (j + 1 == nkt && more) load_qd(n2, hd2, q02);     // next item's Q / dO fragments
      const int kbase = AB_KT * j + 4 * g;
      F dsf;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        const f32x4 ps = xpart[64 * kt], pd = xpart[128 + 64 * kt];
        const f32x4 sf = h == 0 ? s[kt] + ps : ps + s[kt];
        const f32x4 dfull = h == 0 ? d[kt] + pd : pd + d[kt];
        T pv4[4], ds4[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool in = kbase + 16 * kt + r < p.Lk;
          const float pv = in ? __builtin_amdgcn_exp2f(sf[r] * p.scale_log2 - lse2) : 0.f;
          const float ds = p.scale * pv * (dfull[r] - delta);
          pv4[r] = from_f<T>(pv);
          ds4[r] = from_f<T>(ds);
          dsf[kt * 4 + r] = ds4[r];
        }
        const int key = kbase + 16 * kt;
        JMT_DCHECK(qc >= 0 && qc < p.Lq && item < p.nitems);
        if constexpr ((OPT & 16) != 0) {
          pend[kt] = h == 0 ? *(const uint2*)pv4 : *(const uint2*)ds4;
          pend_key[kt] = key;
        } else if (qr < p.Lq && key < p.ldp) {
          if (h == 0) *(uint2*)(prow_p + key) = *(const uint2*)pv4;
          else *(uint2*)(prow_ds + key) = *(const uint2*)ds4;
        }
      }
      if constexpr ((OPT & 16) != 0) pend_on = true;
      // ---- acc[t] += sum_k dS(k) K[k][256h + 16t + 4g + r] (transposed K fragments in
      // double-buffered batches of 4)
      {
        F fa[4], fb[4];
        auto kbatch = [&](F* dst, int b) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int t = 4 * b + i;
            const char* a = kimg + tb8[t & 7] + 256 * (t >> 3);
            const Hf lo = tr_read<Hf>(a);
            const Hf hi = tr_read<Hf>(a + 16384);
            dst[i] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
          }
        };
        kbatch(fa, 0);
#pragma unroll
        for (int b = 0; b < 4; b += 2) {
          kbatch(fb, b + 1);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[4 * b + i] = mfma16(fa[i], dsf, acc[4 * b + i]);
          __builtin_amdgcn_sched_barrier(0);
          if (b + 2 < 4) kbatch(fa, b + 2);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[4 * b + 4 + i] = mfma16(fb[i], dsf, acc[4 * b + 4 + i]);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      if (j + 1 < nkt) {
        wait_vmcnt<0>();                            // tile j+1 landed (and P / dS stores issued)
        lds_barrier();                              // this buffer pair and the slots are free
      }
      buf ^= 1;
    }
    if constexpr ((OPT & 16) != 0) flush();         // the item's last tile
    store_acc_direct<T>(acc, 1.f,
                        (T*)p.dq + (int64_t)n * p.sdq_n + hd * AT_DH + (int64_t)qr * p.sdq_l +
                            256 * h,
                        qr < p.Lq);
    if (!more) break;
    load_o(n2, hd2, q02);                           // O of the next item (Delta), after acc is dead
    lds_barrier();                                  // every wave is done with the last tile's
                                                    // images and exchange slots
    item = nxt; nh = nh2; n = n2; hd = hd2; q0 = q02; kb = kb2; vb = vb2;
  }
}

// ------------------------------------------------------------------ P / dS only (round 6)
// The backward of the jmt_attn_dkdv path: P and dS for jmt_attn_dkdv, which computes dQ = dS K
// as its third product, so this kernel keeps no dQ accumulator.  The freed registers hold the
// WHOLE 512-dim Q and dO rows of a wave (16 fragments each, 128 VGPRs), so:
//  * a block is 8 waves x 16 rows = 128 query rows (the dQ kernel above: 64) — every K / V tile
//    staged into LDS feeds twice the rows, halving the L2 -> LDS fill per FLOP, which bounded it
//    (~64 KiB per 32-key tile per 64-row block at ~4 TB/s chip-wide);
//  * no exchange: each wave contracts all 512 dims itself (S and dP in one MFMA chain each), so
//    no partial-score slots, no pair barrier — one barrier per tile (the K / V buffer turnover);
//  * waves whose 16 rows all lie past Lq (the 44-row tail q-tile of L = 300) skip their MFMAs
//    and stores (wave-uniform), so the tail costs what its rows need.
// Per 32-key tile a wave reads the K and V tiles whole (64 KiB) and issues 64 MFMAs: the LDS
// array (256 B/clk/CU) and the MFMA pipes are both at 2048 cycles per tile at 2 waves/SIMD.
// P / dS leave by 16-B buffer stores, 64 contiguous bytes per row (range-checked rows: the count
// is fixed, so the end-of-tile wait leaves this tile's 2 stores in flight and waits only for the
// next tile's DMA).
// LDS: 2 x (K 32 KiB + V 32 KiB) = 128 KiB.
constexpr int AP_QT = 128;
constexpr int AP_KT = 32;
constexpr int AP_LDS = 4 * AP_KT * AT_ROWB;

// DBG (ablations, timing only, wrong results; JMT_ATTN_PDS_DBG in the diagnostic build): 1 no
// next-item row loads (stale Q / dO / O), 2 no MFMAs, 4 no softmax and no P / dS stores, 8 no
// K / V DMA, 16 softmax computed but not stored, 32 nontemporal stores; 64 phase stamps
// (s_memtime of block gridDim / 2, waves 0 and 4, into p.dq as a uint64 buffer of
// 2 x 256 x 64: phases 8 t + {0 tile start, 1 DMA issued, 2 MFMAs issued, 3 softmax + stores
// issued, 4 end wait, 5 barrier} of the block's first 31 tiles, 255 / 254 item start / end)
// KR: key ranges (attn_common.h KeyRange).  P and dS of keys outside the item's range are written
// as exact zeros in every tile (jmt_attn_dkdv reads whole tiles), so dK / dV of masked keys come
// out as zeros from the zero columns; no tile is skipped and the counted waits are untouched.
// The range of the next item is read where its n2 is formed and carried in two SGPRs.
template <typename T, int DBG = 0, bool SQ = false, bool KR = false>
__global__ __launch_bounds__(512, 2) void attn_bwd_pds_kernel(KrArgs<AttnBwdArgs, KR> p) {
  int tcount = 0;
  auto st = [&](int phase) {
    if constexpr ((DBG & 64) != 0) {
      if (tcount < 31) stamp<true>((uint64_t*)p.dq, 8 * tcount + phase);
    }
  };
  typedef typename Frag16<T>::t F;
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int IMG = AP_KT * AT_ROWB;            // one K or V image (32 KiB)

  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int nqt = (p.Lq + AP_QT - 1) / AP_QT;
  const int nkt = (p.Lk + AP_KT - 1) / AP_KT;
  int item, iend, istride;
  item_range(p.nitems, item, iend, istride);
  if (item >= iend) return;

  int nh = item / nqt, n = nh / p.H, hd = nh % p.H, q0 = (item % nqt) * AP_QT;
  const T* kb = (const T*)p.k + (int64_t)n * p.sk_n + hd * AT_DH;
  const T* vb = (const T*)p.v + (int64_t)n * p.sv_n + hd * AT_DH;

  // lane (li, g): row q0 + 16 w + li, dims 32 ks + 8 g .. +7 of fragment ks
  // The next item's Q / dO go out right after the last tile's MFMAs, its O (Delta only) after
  // the item's last softmax.
  F qf[16], df[16], of[16];
  auto load_qd = [&](int n_, int hd_, int q0_) {
    const int64_t qc_ = min(q0_ + 16 * w + li, p.Lq - 1), coff = (int64_t)hd_ * AT_DH + 8 * g;
    const T* qrow = (const T*)p.q + (int64_t)q_seq<SQ>(p.qs, n_) * p.sq_n + qc_ * p.sq_l + coff;
    const T* drow = (const T*)p.go + (int64_t)n_ * p.sgo_n + qc_ * p.sgo_l + coff;
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
      qf[ks] = *(const F*)(qrow + 32 * ks);
      df[ks] = *(const F*)(drow + 32 * ks);
    }
  };
  auto load_o = [&](int n_, int hd_, int q0_) {
    const int64_t qc_ = min(q0_ + 16 * w + li, p.Lq - 1), coff = (int64_t)hd_ * AT_DH + 8 * g;
    const T* orow = (const T*)p.o + (int64_t)n_ * p.so_n + qc_ * p.so_l + coff;
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) of[ks] = *(const F*)(orow + 32 * ks);
  };
  load_qd(n, hd, q0);
  load_o(n, hd, q0);
  int buf = 0;
  // K / V tile staging: wave w stages rows 4 w .. +3 of both images (one 1-KiB LDS-DMA row per
  // wave-instruction).  Row offsets in 32-bit byte arithmetic from the (n, h) base (the host
  // checks Lk rows fit) and the per-lane swizzled source offsets and LDS addresses computed once:
  // stage_rows' 64-bit row products cost ~25 scalar instructions per DMA on the CU's one scalar
  // unit (1-2.4k cycles of issue per tile, profiles/r06/pds_stamps*.txt)
  const int wu = __builtin_amdgcn_readfirstlane(w);
  const uint32_t lbase = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  unsigned loff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) loff[i] = (unsigned)(lane ^ (((4 * wu + i) & 7) << 1)) << 4;
  const int ldk = (int)(p.sk_l * (int64_t)sizeof(T)), ldv = (int)(p.sv_l * (int64_t)sizeof(T));
  auto stage_tile = [&](int b, const T* kbase, const T* vbase, int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = 4 * wu + i;
      const int src = min(k0 + r, p.Lk - 1);
      const uint32_t dst = lbase + b * 2 * IMG + r * AT_ROWB;
      glds16_at((const char*)kbase + (unsigned)(src * ldk) + loff[i], dst);
      glds16_at((const char*)vbase + (unsigned)(src * ldv) + loff[i], dst + IMG);
    }
  };
  stage_tile(0, kb, vb, 0);
  int kbeg, kend;                                 // valid keys of this item (KR; else [0, Lk))
  key_range<KR>(p, n, p.Lk, kbeg, kend);

  int kb4[4];                                     // ds_read_b128 lane bases (whole row)
#pragma unroll
  for (int m = 0; m < 4; ++m) kb4[m] = row_base(m, li, g, 0);

  while (true) {
    const int qr = q0 + 16 * w + li;
    const int qc = min(qr, p.Lq - 1);
    // wave-uniform (scalar: the branches on it are s_cbranch, not EXEC masks): any row in range
    const bool wact = __builtin_amdgcn_readfirstlane(q0 + 16 * w) < p.Lq;
    const int nxt = item + istride;
    const bool more = nxt < iend;
    const int nh2 = nxt / nqt, n2 = nh2 / p.H, hd2 = nh2 % p.H, q02 = (nxt % nqt) * AP_QT;
    const T* kb2 = (const T*)p.k + (int64_t)n2 * p.sk_n + hd2 * AT_DH;
    const T* vb2 = (const T*)p.v + (int64_t)n2 * p.sv_n + hd2 * AT_DH;
    int kbeg2, kend2;
    key_range<KR>(p, more ? n2 : n, p.Lk, kbeg2, kend2);

    float delta;                                  // rowsum(dO o O) of row qr
    {
      float dp = 0.f;
#pragma unroll
      for (int ks = 0; ks < 16; ++ks)
#pragma unroll
        for (int e = 0; e < 8; ++e) dp += (float)of[ks][e] * (float)df[ks][e];
      delta = pl_pair_sum(dp);
    }
    const float lse2 = p.lse[(int64_t)nh * p.Lq + qc] * 1.4426950408889634f;
    // P / dS of this (n, h), TILE-MAJOR: [key tile jt][query][32 keys] (64-B rows, ldp / 32
    // tiles), so one store instruction writes 16 consecutive rows = 1 KiB contiguous.  Buffer
    // resources over the (n, h) region; rows past Lq get an offset past its end and are dropped
    // by the range check, so every wave issues the same 2 stores per tile.
    const int64_t region = (int64_t)nh * p.Lq * p.ldp;
    const int nbytes = (int)((int64_t)p.Lq * p.ldp * (int64_t)sizeof(T));
    auto mk_rsrc = [&](void* base) {
      const uint64_t ba = (uint64_t)(uintptr_t)((T*)base + region);
      const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)ba);
      const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(ba >> 32));
      return __builtin_amdgcn_make_buffer_rsrc((void*)(((uint64_t)hi << 32) | lo), 0,
                                               __builtin_amdgcn_readfirstlane(nbytes), 0x00020000);
    };
    const auto rs_p = mk_rsrc(p.pbuf);
    const auto rs_ds = mk_rsrc(p.dsbuf);
    const int rowoff = qr * AP_KT;                // elements (used for rows below Lq only)

    wait_vmcnt<0>();                              // tile 0 and this item's rows landed
    lds_barrier();                                // ... for every wave; the previous item's
                                                  // buffers are free
    // One 32-key tile; the last one (LAST) is peeled out of the loop: the next item's Q / dO
    // loads issued inside the loop would be pending at its header for hipcc's wait insertion,
    // which then put a vmcnt(0) before every tile's first MFMA — waiting for the tile's own
    // freshly issued DMA (no load / compute overlap at all).
    auto tile = [&](int j, auto last_c) {
      constexpr bool LAST = decltype(last_c)::value;
      st(0);
      const char* kimg = smem + buf * 2 * IMG;
      const char* vimg = kimg + IMG;
      if ((DBG & 8) == 0 && (!LAST || more))
        stage_tile(buf ^ 1, LAST ? kb2 : kb, LAST ? vb2 : vb, LAST ? 0 : AP_KT * (j + 1));
      st(1);
      // ---- scores s[kt][r] = <row qr, key 32 j + 16 kt + 4 g + r> and dP over all 512 dims
      f32x4 s[2], d[2];
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
        d[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      if ((DBG & 2) == 0 && wact) {   // k-step batches (K and V fragments of key subtiles 0, 1),
                                      // double-buffered
        F fa[4], fb[4];
        auto batch = [&](F* dst, int ks) {
#pragma unroll
          for (int kt = 0; kt < 2; ++kt) {
            const int o = kb4[ks & 3] + 256 * (ks >> 2) + 16384 * kt;
            dst[kt] = *(const F*)(kimg + o);
            dst[2 + kt] = *(const F*)(vimg + o);
          }
        };
        batch(fa, 0);
#pragma unroll
        for (int ks = 0; ks < 16; ks += 2) {
          batch(fb, ks + 1);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int kt = 0; kt < 2; ++kt) {
            s[kt] = mfma16(fa[kt], qf[ks], s[kt]);
            d[kt] = mfma16(fa[2 + kt], df[ks], d[kt]);
          }
          __builtin_amdgcn_sched_barrier(0);
          if (ks + 2 < 16) batch(fa, ks + 2);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int kt = 0; kt < 2; ++kt) {
            s[kt] = mfma16(fb[kt], qf[ks + 1], s[kt]);
            d[kt] = mfma16(fb[2 + kt], df[ks + 1], d[kt]);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      st(2);
      if constexpr (LAST && (DBG & 1) == 0) {
        if (more) load_qd(n2, hd2, q02);          // registers free after the MFMAs
      }
      if ((DBG & 4) == 0 && wact) {
        const int kbase = AP_KT * j + 4 * g;
        uint32_t pk[2][2][2];                     // [P / dS][kt][dword]: 4 keys of subtile kt
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
          T pv4[4], ds4[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int key = kbase + 16 * kt + r;
            const bool in = KR ? (key >= kbeg && key < kend) : key < p.Lk;
            const float pv = in ? __builtin_amdgcn_exp2f(s[kt][r] * p.scale_log2 - lse2) : 0.f;
            pv4[r] = from_f<T>(pv);
            ds4[r] = from_f<T>(p.scale * pv * (d[kt][r] - delta));
          }
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            pk[0][kt][q] = ((const uint32_t*)pv4)[q];
            pk[1][kt][q] = ((const uint32_t*)ds4)[q];
          }
        }
        // subtiles 0 / 1 paired by v_permlane16_swap (store_acc_direct's scheme): lane g then
        // holds the 8 consecutive keys 16 (g & 1) + 8 (g >> 1) .. +7 of the tile: 16 B per lane,
        // a whole 64-B tile row per 4 lanes, 16 rows contiguous (row-major [q][ldp] stores of
        // 32-B / 64-B row pieces took 3/4 of the kernel: 215 -> 57 us without stores,
        // profiles/r06/pds_ablate.txt)
        const int off = qr < p.Lq ? (rowoff + j * p.Lq * AP_KT + 16 * (g & 1) + 8 * (g >> 1)) *
                                        (int)sizeof(T)
                                  : 0x7ffffff0;
        JMT_DCHECK(AP_KT * j + AP_KT <= p.ldp);
#pragma unroll
        for (int a = 0; a < 2; ++a) {
          const auto r0 = __builtin_amdgcn_permlane16_swap(pk[a][0][0], pk[a][1][0], false, false);
          const auto r1 = __builtin_amdgcn_permlane16_swap(pk[a][0][1], pk[a][1][1], false, false);
          const u32x4 v = {r0[0], r1[0], r0[1], r1[1]};
          if constexpr ((DBG & 16) != 0) {
            asm volatile("" ::"v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]));
          } else {
            __builtin_amdgcn_raw_buffer_store_b128(v, a == 0 ? rs_p : rs_ds, off, 0,
                                                   (DBG & 32) ? 2 : 0);
          }
        }
      }
      st(3);
      if constexpr (!LAST) {
        // tile j+1 landed: the 2 stores issued after its DMA may stay in flight
        if ((DBG & 20) == 0 && wact) wait_vmcnt<2>();
        else wait_vmcnt<0>();
        st(4);
        lds_barrier();                            // visible to every wave; buffer `buf` free
        st(5);
      }
      ++tcount;
      buf ^= 1;
    };
    for (int j = 0; j + 1 < nkt; ++j) tile(j, std::false_type{});
    tile(nkt - 1, std::true_type{});
    if (!more) break;
    // after the loop, not in its last iteration: loaded inside, O would be a loop-carried value
    // pinned over every tile (64 VGPRs: the kernel spilled, and each spill reload's vmcnt(0)
    // waited for the tile's DMA right after issuing it)
    if constexpr ((DBG & 1) == 0) load_o(n2, hd2, q02);
    item = nxt; nh = nh2; n = n2; hd = hd2; q0 = q02; kb = kb2; vb = vb2;
    kbeg = kbeg2; kend = kend2;
  }
}

// ------------------------------------------------------------------ forward, whole rows (round 7)
// The forward in the geometry of attn_bwd_pds_kernel: a block is 8 waves x 16 rows = 128 query
// rows, wave w owns rows q0 + 16 w .. +15 over all 512 head dims (Q: 16 fragments, 64 VGPRs; the
// fp32 O accumulator: 32 sub-tiles, 128 VGPRs).  Against attn_fwd_kernel:
//  * no exchange: a wave contracts all 512 dims of its scores itself, so no partial-score slots,
//    no pair barrier and no pair-synchronised softmax — ONE barrier per key tile (the K / V
//    buffer turnover), preceded by the vmcnt that retires the next tile's DMA;
//  * every K / V tile staged into LDS feeds 128 rows (64): half the L2 -> LDS fill per row;
//  * 32-key tiles, K and V double-buffered (tile j+1's DMA issued at the start of tile j, P/dS
//    kernel's stage_tile: inline-asm LDS-DMA, 32-bit row offsets, lane offsets computed once);
//  * waves whose 16 rows all lie past Lq skip their MFMAs, softmax and stores (wave-uniform).
// The scores keep attn_fwd_kernel's summation order: dims 0-255 and 256-511 in separate MFMA
// chains, added lo + hi (bitwise the scores of the 64-row kernel; the four independent chains
// also cover the MFMA dependency latency).  Online softmax with lazy rescaling as there, per
// 32-key tile.  Per tile a wave reads the K and V tiles whole (64 KiB) and issues 64 MFMAs: LDS
// array and MFMA pipes both at 2048 cycles per tile at 2 waves per SIMD.
// LDS: 2 x (K 32 KiB + V 32 KiB) = 128 KiB; 252 VGPRs, no spill, no scratch (both dtypes).
// Tried and dropped: 4-fragment score batches and per-lane 64-bit DMA
// addresses (spilled Q); 2-fragment P V batches (same time); leaving an item's O stores in flight
// across the next item's start (Q loads from inline asm, counted wait: same time).  Ablations
// (profiles/r07/fwd_rows_ablate.txt): the K / V fill and the O stores alone take 131 of the
// 150-158 us of the c3 cross-attention launch — the kernel is bound by the L2 -> LDS fill with
// one 64 KiB tile in flight per CU, not by its MFMAs or LDS reads.
constexpr int AR_QT = 128;
constexpr int AR_KT = 32;
constexpr int AR_LDS = 4 * AR_KT * AT_ROWB;
constexpr int AR_VB = 4;             // V fragments per P V read batch

// DBG (ablations, timing only, wrong results; JMT_ATTN_FWD_ROWS_DBG in the diagnostic build):
// 2 no score reads / MFMAs, 4 no softmax, 8 no K / V DMA after an item's tile 0, 16 no P V reads /
// MFMAs, 32 no O / lse stores.
// KR: key ranges (attn_common.h KeyRange): keys outside the item's range score -inf and get
// probability exactly 0 (selected, not exponentiated: a whole tile left of the range leaves the
// running max at -inf, and exp2(-inf - -inf) is NaN); lse is over the valid keys.  Every tile is
// still staged and multiplied (masking only; skipping tiles outside the range is not built).
template <typename T, int DBG = 0, bool SQ = false, bool KR = false>
__global__ __launch_bounds__(512, 2) void attn_fwd_rows_kernel(KrArgs<AttnFwdArgs, KR> p) {
  typedef typename Frag16<T>::t F;
  typedef typename Frag16<T>::h Hf;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int IMG = AR_KT * AT_ROWB;            // one K or V image (32 KiB)

  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int nqt = (p.Lq + AR_QT - 1) / AR_QT;
  const int nkt = (p.Lk + AR_KT - 1) / AR_KT;
  int item, iend, istride;
  item_range(p.nitems, item, iend, istride);
  if (item >= iend) return;

  int nh = item / nqt, n = nh / p.H, hd = nh % p.H, q0 = (item % nqt) * AR_QT;
  const T* kb = (const T*)p.k + (int64_t)n * p.sk_n + hd * AT_DH;
  const T* vb = (const T*)p.v + (int64_t)n * p.sv_n + hd * AT_DH;

  // lane (li, g): row q0 + 16 w + li, dims 32 ks + 8 g .. +7 of fragment ks
  F qf[16];
  auto load_q = [&](int n_, int hd_, int q0_) {
    const T* qrow = (const T*)p.q + (int64_t)q_seq<SQ>(p.qs, n_) * p.sq_n + hd_ * AT_DH +
                    (int64_t)min(q0_ + 16 * w + li, p.Lq - 1) * p.sq_l + 8 * g;
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) qf[ks] = *(const F*)(qrow + 32 * ks);
  };
  load_q(n, hd, q0);
  int buf = 0;
  // K / V tile staging as attn_bwd_pds_kernel: wave w stages rows 4 w .. +3 of both images, row
  // offsets in 32-bit byte arithmetic from the (n, h) base (the host checks Lk rows fit)
  const int wu = __builtin_amdgcn_readfirstlane(w);
  const uint32_t lbase = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  unsigned loff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) loff[i] = (unsigned)(lane ^ (((4 * wu + i) & 7) << 1)) << 4;
  const int ldk = (int)(p.sk_l * (int64_t)sizeof(T)), ldv = (int)(p.sv_l * (int64_t)sizeof(T));
  auto stage_tile = [&](int b, const T* kbase, const T* vbase, int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = 4 * wu + i;
      const int src = min(k0 + r, p.Lk - 1);
      JMT_DCHECK(src >= 0 && src < p.Lk);
      const uint32_t dst = lbase + b * 2 * IMG + r * AT_ROWB;
      glds16_sv((const char*)kbase + (unsigned)(src * ldk), loff[i], dst);
      glds16_sv((const char*)vbase + (unsigned)(src * ldv), loff[i], dst + IMG);
    }
  };
  stage_tile(0, kb, vb, 0);
  int kbeg, kend;                                 // valid keys of this item (KR; else [0, Lk))
  key_range<KR>(p, n, p.Lk, kbeg, kend);
  // Lane bases of the fragment reads: row_base(m) = row_base(0) ^ (m << 6) and tr_base(c) =
  // tr_base(0) ^ (c << 5) (the swizzle XOR and m / c sit in the same chunk bits), formed by one
  // VALU XOR in front of the reads that use them instead of living in 12 registers over the
  // whole kernel (the O accumulator and Q leave 64 for everything else); asm volatile keeps
  // hipcc from hoisting them back out of the tile loop.
  const int kb0 = row_base(0, li, g, 0), tb0 = tr_base(0, li, g, 0);
  auto lane_base = [](int base, int bits) __attribute__((always_inline)) {
#if !defined(__OPTIMIZE__)
    return base ^ bits;
#else
    int r;
    asm volatile("v_xor_b32 %0, %2, %1" : "=v"(r) : "v"(base), "i"(bits));
    return r;
#endif
  };

  while (true) {
    const int qr = q0 + 16 * w + li;
    // wave-uniform (scalar branches, not EXEC masks): any row of this wave in range
    const bool wact = __builtin_amdgcn_readfirstlane(q0 + 16 * w) < p.Lq;
    const int nxt = item + istride;
    const bool more = nxt < iend;
    const int nh2 = nxt / nqt, n2 = nh2 / p.H, hd2 = nh2 % p.H, q02 = (nxt % nqt) * AR_QT;
    const T* kb2 = (const T*)p.k + (int64_t)n2 * p.sk_n + hd2 * AT_DH;
    const T* vb2 = (const T*)p.v + (int64_t)n2 * p.sv_n + hd2 * AT_DH;
    int kbeg2, kend2;
    key_range<KR>(p, more ? n2 : n, p.Lk, kbeg2, kend2);

    f32x4 o[32];
#pragma unroll
    for (int t = 0; t < 32; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;

    wait_vmcnt<0>();                              // tile 0 and this item's Q landed (and the
                                                  // previous item's O stores left)
    // a use of Q here: hipcc's own wait for the Q loads goes in front of it, outside the tile
    // loop (inside, it would drain each tile's freshly issued DMA before the first MFMA)
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) asm volatile("" : "+v"(qf[ks]));
    lds_barrier();                                // ... for every wave; the previous item's
                                                  // buffers are free
    // One 32-key tile; the last one (LAST) is peeled out of the loop so that the next item's Q
    // loads are not pending at the loop header (attn_bwd_pds_kernel).
    auto tile = [&](int j, auto last_c) {
      constexpr bool LAST = decltype(last_c)::value;
      const char* kimg = smem + buf * 2 * IMG;
      const char* vimg = kimg + IMG;
      if ((!LAST && (DBG & 8) == 0) || (LAST && more))
        stage_tile(buf ^ 1, LAST ? kb2 : kb, LAST ? vb2 : vb, LAST ? 0 : AR_KT * (j + 1));
      // ---- scores <row qr, key 32 j + 16 kt + 4 g + r>: dims 0-255 into sl, 256-511 into sh
      f32x4 sl[2], sh[2];
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        sl[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
        sh[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      if ((DBG & 2) == 0 && wact) {   // batches of 2 K fragments (key subtiles 0, 1 of one k-step, dims 0-255 and
                    // 256-511 alternating), double-buffered: the next batch is in flight while
                    // the 2 MFMAs of this one run (4-fragment batches spill Q)
        F fa[2], fb[2];
        auto batch = [&](F* dst, const char* a) {
#pragma unroll
          for (int kt = 0; kt < 2; ++kt) dst[kt] = *(const F*)(a + 16384 * kt);
        };
        const char* a = kimg + lane_base(kb0, 0);
        batch(fa, a);
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
          batch(fb, a + 512);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int kt = 0; kt < 2; ++kt) sl[kt] = mfma16(fa[kt], qf[ks], sl[kt]);
          __builtin_amdgcn_sched_barrier(0);
          if (ks + 1 < 8) {
            a = kimg + lane_base(kb0, ((ks + 1) & 3) << 6) + 256 * ((ks + 1) >> 2);
            batch(fa, a);
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int kt = 0; kt < 2; ++kt) sh[kt] = mfma16(fb[kt], qf[ks + 8], sh[kt]);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      if constexpr (LAST) {
        if (more) load_q(n2, hd2, q02);           // registers free after the score MFMAs
      }
      if (wact) {
        F pf;
        if constexpr ((DBG & 4) != 0) {
#pragma unroll
          for (int e = 0; e < 8; ++e) pf[e] = from_f<T>(0.f);
#pragma unroll
          for (int kt = 0; kt < 2; ++kt)
            asm volatile("" ::"v"(sl[kt][0]), "v"(sl[kt][3]), "v"(sh[kt][0]), "v"(sh[kt][3]));
        } else {
        // ---- online softmax of the tile (lazy rescale: attn_fwd_kernel)
        const int kbase = AR_KT * j + 4 * g;
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
          const f32x4 full = sl[kt] + sh[kt];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int key = kbase + 16 * kt + r;
            const bool in = KR ? (key >= kbeg && key < kend) : key < p.Lk;
            const float x = in ? full[r] * p.scale_log2 : -INFINITY;
            sl[kt][r] = x;
            mx = fmaxf(mx, x);
          }
        }
        mx = pl_pair_max(mx);
        if constexpr (!KR) {
        if (__any(mx > m_run + 8.f)) {
          const float m_new = fmaxf(m_run, mx);
          const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
          m_run = m_new;
          l_run *= alpha;
#pragma unroll
          for (int t = 0; t < 32; ++t) o[t] *= alpha;
        }
        } else {
        // The vote is the wave's, for its 16 query rows together, so a row's rounding depends on
        // its neighbours' scores.  With ranges, a query row whose own index is a masked key (a
        // padded frame where queries and keys share the axis) takes no part in the vote of the
        // other rows: those rescale only when one of them asks (else alpha = 1, a bitwise no-op),
        // the masked-index rows whenever the branch is entered.  Any such schedule is a correct
        // lazy rescale (a row that needs it always gets it); this one keeps the values at valid
        // frames independent of what the padded frames hold, and with nothing masked it is the
        // vote above (bitwise the kernel without ranges).
        const bool need = mx > m_run + 8.f;
        if (__any(need)) {
          const int qc = min(qr, p.Lq - 1);         // rows past Lq repeat row Lq - 1
          const bool qin = !(qc < kbeg || (qc >= kend && qc < p.Lk));
          const bool apply = !qin || __any(need && qin);
          const float m_new = apply ? fmaxf(m_run, mx) : m_run;
          const float alpha = apply ? __builtin_amdgcn_exp2f(m_run - m_new) : 1.f;
          m_run = m_new;
          l_run *= alpha;
#pragma unroll
          for (int t = 0; t < 32; ++t) o[t] *= alpha;
        }
        }
        float ls = 0.f;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float pv = __builtin_amdgcn_exp2f(sl[kt][r] - m_run);
            if constexpr (KR) pv = sl[kt][r] == -INFINITY ? 0.f : pv;
            ls += pv;
            pf[kt * 4 + r] = from_f<T>(pv);
          }
        l_run += ls;
        }
        if constexpr ((DBG & 16) != 0) {
          asm volatile("" ::"v"(pf));
        } else {
        // ---- o[t] += sum_k P(k) V[k][16 t + 4 g + r]: transposed fragment reads of the V image
        // in double-buffered batches of NB fragments
        constexpr int NB = AR_VB;
        F fa[NB], fb[NB];
        auto vbatch = [&](F* dst, int b) {
#pragma unroll
          for (int i = 0; i < NB; ++i) {
            const int t = NB * b + i;
            const char* a = vimg + lane_base(tb0, (t & 7) << 5) + 256 * (t >> 3);
            const Hf lo = tr_read<Hf>(a);
            const Hf hi = tr_read<Hf>(a + 16384);
            dst[i] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
          }
        };
        vbatch(fa, 0);
#pragma unroll
        for (int b = 0; b < 32 / NB; b += 2) {
          vbatch(fb, b + 1);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int i = 0; i < NB; ++i) o[NB * b + i] = mfma16(fa[i], pf, o[NB * b + i]);
          __builtin_amdgcn_sched_barrier(0);
          if (b + 2 < 32 / NB) vbatch(fa, b + 2);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int i = 0; i < NB; ++i)
            o[NB * (b + 1) + i] = mfma16(fb[i], pf, o[NB * (b + 1) + i]);
          __builtin_amdgcn_sched_barrier(0);
        }
        }
      }
      if constexpr (!LAST) {
        wait_vmcnt<0>();                          // tile j+1 landed
        lds_barrier();                            // visible to every wave; buffer `buf` free
      }
      buf ^= 1;
    };
    for (int j = 0; j + 1 < nkt; ++j) tile(j, std::false_type{});
    tile(nkt - 1, std::true_type{});
    if constexpr ((DBG & 32) != 0) {
#pragma unroll
      for (int t = 0; t < 32; ++t) asm volatile("" ::"v"(o[t]));
      asm volatile("" ::"v"(l_run), "v"(m_run));
    } else if (wact) {
      const float lt = pl_pair_sum(l_run);
      JMT_DCHECK(item < p.nitems && n * p.H + hd == nh);
      if (qr < p.Lq && g == 0 && p.lse)
        p.lse[(int64_t)nh * p.Lq + qr] =
            (m_run + __builtin_amdgcn_logf(lt)) * 0.69314718055994531f;
      T* orow = (T*)p.o + (int64_t)n * p.so_n + hd * AT_DH + (int64_t)qr * p.so_l;
      store_acc_direct<T>(o, 1.f / lt, orow, qr < p.Lq);
      store_acc_direct<T>(o + 16, 1.f / lt, orow + 256, qr < p.Lq);
    }
    if (!more) break;
    item = nxt; nh = nh2; n = n2; hd = hd2; q0 = q02; kb = kb2; vb = vb2;
    kbeg = kbeg2; kend = kend2;
  }
}

// ---- the kernels' ranges (host only: sizes and row strides, no pointer).  The entry points
// validate with these and the jmt_attn_*_ok exports answer from them, so a limit is written once.
// qt: query rows per item of the kernel the caller launches (the item count must fit an int)
static bool sizes_ok(int N, int H, int Lq, int Lk, int qt) {
  return N > 0 && H > 0 && Lq > 0 && Lk > 0 &&
         (int64_t)N * H * ((Lq + qt - 1) / qt) < (1LL << 31);
}
// L rows of row stride s (16-bit elements) within 32-bit byte offsets
static bool rows_fit(int64_t L, int64_t s) { return L * s * 2 < (1LL << 31); }

// nullptr when the P / dS kernel (jmt_attn_bwd with dq == NULL) takes these sizes and strides,
// else what is out of range
static const char* pds_range(int N, int H, int Lq, int Lk, int64_t ldp, int64_t sk_l,
                             int64_t sv_l) {
  if (!sizes_ok(N, H, Lq, Lk, AP_QT)) return "bad sizes";
  if (ldp < (int64_t)(Lk + AP_KT - 1) / AP_KT * AP_KT || ldp % AP_KT != 0)
    return "ldp must be a multiple of 32 covering Lk";
  if ((int64_t)(Lq + AP_QT) * ldp * 2 >= (1LL << 30))
    return "Lq + 128 rows of ldp 16-bit values must stay below 1 GiB";
  if (!rows_fit(Lk, sk_l) || !rows_fit(Lk, sv_l)) return "Lk K / V rows must stay below 2 GiB";
  return nullptr;
}

static int check_common(const char* name, int N, int H, int Lq, int Lk, int qt,
                        const void* const* ptrs, int nptr, const int64_t* strides, int nstr) {
  JMT_CHECK_ARG(sizes_ok(N, H, Lq, Lk, qt), "%s: bad sizes", name);
  for (int i = 0; i < nptr; ++i)
    JMT_CHECK_ARG(ptrs[i] != nullptr && ((uintptr_t)ptrs[i] & 15) == 0,
                  "%s: operand %d null or not 16-B aligned", name, i);
  for (int i = 0; i < nstr; ++i)
    JMT_CHECK_ARG(strides[i] % 8 == 0, "%s: stride %d not a multiple of 8 elements", name, i);
  return JMT_OK;
}

}  // namespace jmt

using namespace jmt;

[[maybe_unused]] static void* g_stamps = nullptr;

// Schedule options of the bf16 / fp16 kernels (OPT bits, compile time; forward: 1 permlane
// reductions, 2 setprio for waves 4-7, 4 interleaved K-tile DMA, 8 split exponentials;
// backward: 1, 2, 4, 16 deferred P / dS stores).  The measured-fastest combination is the only
// one compiled (profiles/r03_attn_opt_ab.jsonl, interleaved A/B at the c3 launches: forward
// 1|2|8, backward 1|2|4).
constexpr int ATTN_FWD_OPT = 11;
constexpr int ATTN_BWD_OPT = 7;

// one block per CU (the 160 KiB of LDS admit one), rounded down to a multiple of 8 (XCDs), when
// there are more items than CUs; otherwise one block per item
static unsigned persistent_grid(int nitems) {
  static int ncu = 0;
  if (ncu == 0) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v < 8)
      v = 8;
    ncu = v / 8 * 8;
    const char* e = getenv("JMT_ATTN_PERSIST");   // dev A/B switch: 0 = one block per item
    if (e && e[0] == '0') ncu = 1 << 30;
  }
  return (unsigned)(nitems > ncu ? ncu : nitems);
}

// diagnostic: route jmt_attn_fwd (bf16) through the phase-stamped kernel, stamps into `buf`
// (2 x 256 x 64 uint64); NULL turns it off.  Only in the diagnostic build (make diag,
// -DJMT_DIAG=1); not part of include/jmt.h (dev tool).
extern "C" int jmt_attn_set_stamps(void* buf) {
#if JMT_DIAG
  g_stamps = buf;
  return JMT_OK;
#else
  return buf ? set_error(JMT_ERR_UNSUPPORTED, "jmt_attn_set_stamps: diagnostic build only "
                                              "(make diag)") : JMT_OK;
#endif
}

// dev A/B switch of the forward: JMT_ATTN_FWD_ROWS=0 (read once) keeps every shape on the 64-row
// attn_fwd_kernel; jmt_attn_set_fwd_rows(0 / 1) overrides it in-process (tests and benchmarks
// that compare the two kernels), -1 returns to the environment's choice.  Not part of
// include/jmt.h (dev tool, as jmt_attn_set_stamps).
static int g_fwd_rows = -1;
static bool fwd_rows_on() {
  static const bool env_on = [] {
    const char* e = getenv("JMT_ATTN_FWD_ROWS");
    return !(e && e[0] == '0');
  }();
  return g_fwd_rows < 0 ? env_on : g_fwd_rows != 0;
}
extern "C" int jmt_attn_set_fwd_rows(int on) {
  g_fwd_rows = on < 0 ? -1 : (on != 0);
  return JMT_OK;
}

extern "C" int jmt_attn_supported(int dt, int dh) {
  return (dt == JMT_BF16 || dt == JMT_F16) && dh == AT_DH;
}

// The whole-row kernel (128-row items) takes Lq > 64 when its 32-bit K / V row offsets fit;
// Lq <= 64 stays on the 64-row kernel, whose arithmetic jmt_attn_short_fwd reproduces bit for
// bit (include/jmt.h).
static bool fwd_rows(int Lq, int Lk, int64_t sk_l, int64_t sv_l) {
  return fwd_rows_on() && Lq > AT_QT && rows_fit(Lk, sk_l) && rows_fit(Lk, sv_l);
}

extern "C" int jmt_attn_fwd_rows_ok(int N, int H, int Lq, int Lk, int64_t sk_l, int64_t sv_l) {
  return fwd_rows(Lq, Lk, sk_l, sv_l) && sizes_ok(N, H, Lq, Lk, AR_QT);
}

extern "C" int jmt_attn_bwd_pds_ok(int N, int H, int Lq, int Lk, int64_t ldp, int64_t sk_l,
                                   int64_t sv_l) {
  return pds_range(N, H, Lq, Lk, ldp, sk_l, sv_l) == nullptr;
}

// jmt_attn_fwd (qs == NULL) and jmt_attn_fwd_sq (qs: the packed query table; the whole-row
// kernel only); kr: the key range table of the *_kr forms (the whole-row kernel only)
static int attn_fwd_impl(int dt, int N, int H, int Lq, int Lk, int dh, const void* q,
                         int64_t sq_l, int64_t sq_n, const void* k, int64_t sk_l, int64_t sk_n,
                         const void* v, int64_t sv_l, int64_t sv_n, void* o, int64_t so_l,
                         int64_t so_n, float scale, float* lse, const QShare* qs,
                         const KeyRange* kr, void* stream) {
  if (N == 0 || Lq == 0) return JMT_OK;
  if (!jmt_attn_supported(dt, dh))
    return set_error(JMT_ERR_UNSUPPORTED, "jmt_attn_fwd: dtype %d / head dim %d not supported",
                     dt, dh);
  const void* ptrs[] = {q, k, v, o};
  const int64_t strides[] = {sq_l, sq_n, sk_l, sk_n, sv_l, sv_n, so_l, so_n};
  const bool rows = fwd_rows(Lq, Lk, sk_l, sv_l);
  if (qs && !rows)
    return set_error(JMT_ERR_UNSUPPORTED, "jmt_attn_fwd_sq: the whole-row kernel only (Lq > %d, "
                                          "Lk K / V rows below 2 GiB, JMT_ATTN_FWD_ROWS on)",
                     AT_QT);
  if (kr && !rows)
    return set_error(JMT_ERR_UNSUPPORTED, "jmt_attn_fwd_kr: the whole-row kernel only (Lq > %d, "
                                          "Lk K / V rows below 2 GiB, JMT_ATTN_FWD_ROWS on)",
                     AT_QT);
  const int qt = rows ? AR_QT : AT_QT;
  int rc = check_common("jmt_attn_fwd", N, H, Lq, Lk, qt, ptrs, 4, strides, 8);
  if (rc != JMT_OK) return rc;
  if (kr && (rc = key_range_check("jmt_attn_fwd_kr", N, kr->tab, kr->mod)) != JMT_OK) return rc;
  AttnFwdArgs a = {};
  if (qs) a.qs = *qs;
  a.q = q; a.k = k; a.v = v; a.o = o; a.lse = lse;
  a.sq_l = sq_l; a.sq_n = sq_n; a.sk_l = sk_l; a.sk_n = sk_n; a.sv_l = sv_l; a.sv_n = sv_n;
  a.so_l = so_l; a.so_n = so_n;
  a.Lq = Lq; a.Lk = Lk; a.H = H;
  a.scale_log2 = scale * 1.4426950408889634f;
  hipStream_t st = as_stream(stream);
  a.nitems = ((Lq + qt - 1) / qt) * N * H;
  const dim3 grid(persistent_grid(a.nitems));
  const char* name = qs ? "jmt_attn_fwd_sq" : "jmt_attn_fwd";
#if JMT_DIAG
  static const int dbg =
      getenv("JMT_ATTN_FWD_ROWS_DBG") ? atoi(getenv("JMT_ATTN_FWD_ROWS_DBG")) : 0;
  if (rows && dbg && dt == JMT_BF16) {
#define JMT_ROWS_DBG(D) \
  case D: attn_launch<attn_fwd_rows_kernel<__bf16, D>, AR_LDS>(grid, st, a); break;
    switch (dbg) {
      JMT_ROWS_DBG(2) JMT_ROWS_DBG(4) JMT_ROWS_DBG(8) JMT_ROWS_DBG(16) JMT_ROWS_DBG(32)
      JMT_ROWS_DBG(18) JMT_ROWS_DBG(22) JMT_ROWS_DBG(54) JMT_ROWS_DBG(62)
      default: return set_error(JMT_ERR_ARG, "JMT_ATTN_FWD_ROWS_DBG=%d not built", dbg);
    }
#undef JMT_ROWS_DBG
    JMT_LAUNCH_CHECK("jmt_attn_fwd");
    return JMT_OK;
  }
  if (!rows && g_stamps && dt == JMT_BF16) {   // diagnostic: phase stamps (jmt_attn_set_stamps)
    a.stamps = (uint64_t*)g_stamps;
    attn_launch<attn_fwd_kernel<__bf16, true, ATTN_FWD_OPT>, AF_LDS>(grid, st, a);
    JMT_LAUNCH_CHECK("jmt_attn_fwd");
    return JMT_OK;
  }
#endif
  by_elem(dt, [&](auto e) {
    using T = typename decltype(e)::type;
    if (!rows) attn_launch<attn_fwd_kernel<T, false, ATTN_FWD_OPT>, AF_LDS>(grid, st, a);
    else if (kr) {
      WithKeyRange<AttnFwdArgs> ak;
      static_cast<AttnFwdArgs&>(ak) = a;
      ak.kr = *kr;
      if (qs) attn_launch<attn_fwd_rows_kernel<T, 0, true, true>, AR_LDS>(grid, st, ak);
      else attn_launch<attn_fwd_rows_kernel<T, 0, false, true>, AR_LDS>(grid, st, ak);
    }
    else if (qs) attn_launch<attn_fwd_rows_kernel<T, 0, true>, AR_LDS>(grid, st, a);
    else attn_launch<attn_fwd_rows_kernel<T>, AR_LDS>(grid, st, a);
  });
  JMT_LAUNCH_CHECK(name);
  return JMT_OK;
}

extern "C" int jmt_attn_fwd(int dt, int N, int H, int Lq, int Lk, int dh, const void* q,
                            int64_t sq_l, int64_t sq_n, const void* k, int64_t sk_l, int64_t sk_n,
                            const void* v, int64_t sv_l, int64_t sv_n, void* o, int64_t so_l,
                            int64_t so_n, float scale, float* lse, void* stream) {
  return attn_fwd_impl(dt, N, H, Lq, Lk, dh, q, sq_l, sq_n, k, sk_l, sk_n, v, sv_l, sv_n, o, so_l,
                       so_n, scale, lse, nullptr, nullptr, stream);
}

extern "C" int jmt_attn_fwd_kr(int dt, int N, int H, int Lq, int Lk, int dh, const void* q,
                               int64_t sq_l, int64_t sq_n, const void* k, int64_t sk_l,
                               int64_t sk_n, const void* v, int64_t sv_l, int64_t sv_n, void* o,
                               int64_t so_l, int64_t so_n, float scale, float* lse,
                               const int* kr, int kr_mod, void* stream) {
  const KeyRange r = {kr, kr_mod};
  return attn_fwd_impl(dt, N, H, Lq, Lk, dh, q, sq_l, sq_n, k, sk_l, sk_n, v, sv_l, sv_n, o, so_l,
                       so_n, scale, lse, nullptr, &r, stream);
}

extern "C" int jmt_attn_fwd_sq(int dt, int N, int H, int Lq, int Lk, int dh, const void* q,
                               int64_t sq_l, int64_t sq_n, const void* k, int64_t sk_l,
                               int64_t sk_n, const void* v, int64_t sv_l, int64_t sv_n, void* o,
                               int64_t so_l, int64_t so_n, float scale, float* lse, int spp,
                               const int* qtab, int npair, void* stream) {
  if (N == 0 || Lq == 0) return JMT_OK;
  if (!jmt_attn_supported(dt, dh))
    return set_error(JMT_ERR_UNSUPPORTED, "jmt_attn_fwd_sq: dtype %d / head dim %d not supported",
                     dt, dh);
  QShare qs = {};
  int rc = qshare_pack("jmt_attn_fwd_sq", N, spp, qtab, npair, &qs);
  if (rc != JMT_OK) return rc;
  return attn_fwd_impl(dt, N, H, Lq, Lk, dh, q, sq_l, sq_n, k, sk_l, sk_n, v, sv_l, sv_n, o, so_l,
                       so_n, scale, lse, &qs, nullptr, stream);
}

extern "C" int jmt_attn_fwd_sq_kr(int dt, int N, int H, int Lq, int Lk, int dh, const void* q,
                                  int64_t sq_l, int64_t sq_n, const void* k, int64_t sk_l,
                                  int64_t sk_n, const void* v, int64_t sv_l, int64_t sv_n, void* o,
                                  int64_t so_l, int64_t so_n, float scale, float* lse, int spp,
                                  const int* qtab, int npair, const int* kr, int kr_mod,
                                  void* stream) {
  if (N == 0 || Lq == 0) return JMT_OK;
  if (!jmt_attn_supported(dt, dh))
    return set_error(JMT_ERR_UNSUPPORTED,
                     "jmt_attn_fwd_sq_kr: dtype %d / head dim %d not supported", dt, dh);
  QShare qs = {};
  int rc = qshare_pack("jmt_attn_fwd_sq_kr", N, spp, qtab, npair, &qs);
  if (rc != JMT_OK) return rc;
  const KeyRange r = {kr, kr_mod};
  return attn_fwd_impl(dt, N, H, Lq, Lk, dh, q, sq_l, sq_n, k, sk_l, sk_n, v, sv_l, sv_n, o, so_l,
                       so_n, scale, lse, &qs, &r, stream);
}

// jmt_attn_bwd (qs == NULL) and jmt_attn_bwd_sq (qs: the packed query table; dq == NULL only);
// kr: the key range table of the *_kr forms (dq == NULL only)
static int attn_bwd_impl(int dt, int N, int H, int Lq, int Lk, int dh, const void* go,
                         int64_t sgo_l, int64_t sgo_n, const void* o, int64_t so_l, int64_t so_n,
                         const void* q, int64_t sq_l, int64_t sq_n, const void* k, int64_t sk_l,
                         int64_t sk_n, const void* v, int64_t sv_l, int64_t sv_n,
                         const float* lse, void* p_out, void* ds_out, int64_t ldp, void* dq,
                         int64_t sdq_l, int64_t sdq_n, float scale, const QShare* qs,
                         const KeyRange* kr, void* stream) {
  if (N == 0 || Lq == 0) return JMT_OK;
  if (!jmt_attn_supported(dt, dh))
    return set_error(JMT_ERR_UNSUPPORTED, "jmt_attn_bwd: dtype %d / head dim %d not supported",
                     dt, dh);
  const void* ptrs[] = {go, o, q, k, v, p_out, ds_out, dq};
  const int64_t strides[] = {sgo_l, sgo_n, so_l, so_n, sq_l, sq_n, sk_l, sk_n, sv_l, sv_n, ldp,
                             sdq_l, sdq_n};
  const bool pds = dq == nullptr;                 // P / dS only: dQ left to jmt_attn_dkdv
  if (kr && !pds)
    return set_error(JMT_ERR_UNSUPPORTED, "jmt_attn_bwd_kr: the P / dS kernel only (dq = NULL)");
  const int qt = pds ? AP_QT : AT_QT;
  int rc = check_common("jmt_attn_bwd", N, H, Lq, Lk, qt, ptrs, pds ? 7 : 8, strides,
                        pds ? 11 : 13);
  if (rc != JMT_OK) return rc;
  JMT_CHECK_ARG(lse && ldp >= Lk, "jmt_attn_bwd: lse missing or ldp < Lk");
  if (pds) {
    const char* why = pds_range(N, H, Lq, Lk, ldp, sk_l, sv_l);
    JMT_CHECK_ARG(!why, "jmt_attn_bwd (dq = NULL): %s", why);
  }
  if (kr && (rc = key_range_check("jmt_attn_bwd_kr", N, kr->tab, kr->mod)) != JMT_OK) return rc;
  AttnBwdArgs a = {};
  if (qs) a.qs = *qs;
  a.go = go; a.o = o; a.q = q; a.k = k; a.v = v; a.lse = lse;
  a.pbuf = p_out; a.dsbuf = ds_out; a.dq = dq;
  a.sgo_l = sgo_l; a.sgo_n = sgo_n; a.so_l = so_l; a.so_n = so_n; a.sq_l = sq_l; a.sq_n = sq_n;
  a.sk_l = sk_l; a.sk_n = sk_n; a.sv_l = sv_l; a.sv_n = sv_n;
  if (!pds) { a.sdq_l = sdq_l; a.sdq_n = sdq_n; }
  a.ldp = ldp;
  a.Lq = Lq; a.Lk = Lk; a.H = H;
  a.scale = scale;
  a.scale_log2 = scale * 1.4426950408889634f;
  a.nitems = ((Lq + qt - 1) / qt) * N * H;
  const dim3 grid(persistent_grid(a.nitems));
  hipStream_t st = as_stream(stream);
  const char* name = qs ? "jmt_attn_bwd_sq" : "jmt_attn_bwd";
#if JMT_DIAG
  static const int dbg = getenv("JMT_ATTN_PDS_DBG") ? atoi(getenv("JMT_ATTN_PDS_DBG")) : 0;
  if (pds && dbg && dt == JMT_BF16) {
    if (dbg & 64) a.dq = g_stamps;              // the stamps buffer (jmt_attn_set_stamps)
#define JMT_PDS_DBG(D) \
  case D: attn_launch<attn_bwd_pds_kernel<__bf16, D>, AP_LDS>(grid, st, a); break;
    switch (dbg) {
      JMT_PDS_DBG(1) JMT_PDS_DBG(2) JMT_PDS_DBG(3) JMT_PDS_DBG(4) JMT_PDS_DBG(6)
      JMT_PDS_DBG(7) JMT_PDS_DBG(8) JMT_PDS_DBG(15) JMT_PDS_DBG(16) JMT_PDS_DBG(32)
      JMT_PDS_DBG(17) JMT_PDS_DBG(18) JMT_PDS_DBG(64)
      default: return set_error(JMT_ERR_ARG, "JMT_ATTN_PDS_DBG=%d not built", dbg);
    }
#undef JMT_PDS_DBG
    JMT_LAUNCH_CHECK("jmt_attn_bwd");
    return JMT_OK;
  }
#endif
  by_elem(dt, [&](auto e) {
    using T = typename decltype(e)::type;
    if (!pds) attn_launch<attn_bwd_kernel<T, ATTN_BWD_OPT>, AB_LDS>(grid, st, a);
    else if (kr) {
      WithKeyRange<AttnBwdArgs> ak;
      static_cast<AttnBwdArgs&>(ak) = a;
      ak.kr = *kr;
      if (qs) attn_launch<attn_bwd_pds_kernel<T, 0, true, true>, AP_LDS>(grid, st, ak);
      else attn_launch<attn_bwd_pds_kernel<T, 0, false, true>, AP_LDS>(grid, st, ak);
    }
    else if (qs) attn_launch<attn_bwd_pds_kernel<T, 0, true>, AP_LDS>(grid, st, a);
    else attn_launch<attn_bwd_pds_kernel<T>, AP_LDS>(grid, st, a);
  });
  JMT_LAUNCH_CHECK(name);
  return JMT_OK;
}

extern "C" int jmt_attn_bwd(int dt, int N, int H, int Lq, int Lk, int dh, const void* go,
                            int64_t sgo_l, int64_t sgo_n, const void* o, int64_t so_l,
                            int64_t so_n, const void* q, int64_t sq_l, int64_t sq_n,
                            const void* k, int64_t sk_l, int64_t sk_n, const void* v,
                            int64_t sv_l, int64_t sv_n, const float* lse, void* p_out,
                            void* ds_out, int64_t ldp, void* dq, int64_t sdq_l, int64_t sdq_n,
                            float scale, void* stream) {
  return attn_bwd_impl(dt, N, H, Lq, Lk, dh, go, sgo_l, sgo_n, o, so_l, so_n, q, sq_l, sq_n, k,
                       sk_l, sk_n, v, sv_l, sv_n, lse, p_out, ds_out, ldp, dq, sdq_l, sdq_n, scale,
                       nullptr, nullptr, stream);
}

// the dq == NULL form only (P / dS for jmt_attn_dkdv)
extern "C" int jmt_attn_bwd_kr(int dt, int N, int H, int Lq, int Lk, int dh, const void* go,
                               int64_t sgo_l, int64_t sgo_n, const void* o, int64_t so_l,
                               int64_t so_n, const void* q, int64_t sq_l, int64_t sq_n,
                               const void* k, int64_t sk_l, int64_t sk_n, const void* v,
                               int64_t sv_l, int64_t sv_n, const float* lse, void* p_out,
                               void* ds_out, int64_t ldp, float scale, const int* kr, int kr_mod,
                               void* stream) {
  const KeyRange r = {kr, kr_mod};
  return attn_bwd_impl(dt, N, H, Lq, Lk, dh, go, sgo_l, sgo_n, o, so_l, so_n, q, sq_l, sq_n, k,
                       sk_l, sk_n, v, sv_l, sv_n, lse, p_out, ds_out, ldp, nullptr, 0, 0, scale,
                       nullptr, &r, stream);
}

extern "C" int jmt_attn_bwd_sq(int dt, int N, int H, int Lq, int Lk, int dh, const void* go,
                               int64_t sgo_l, int64_t sgo_n, const void* o, int64_t so_l,
                               int64_t so_n, const void* q, int64_t sq_l, int64_t sq_n,
                               const void* k, int64_t sk_l, int64_t sk_n, const void* v,
                               int64_t sv_l, int64_t sv_n, const float* lse, void* p_out,
                               void* ds_out, int64_t ldp, float scale, int spp, const int* qtab,
                               int npair, void* stream) {
  if (N == 0 || Lq == 0) return JMT_OK;
  if (!jmt_attn_supported(dt, dh))
    return set_error(JMT_ERR_UNSUPPORTED, "jmt_attn_bwd_sq: dtype %d / head dim %d not supported",
                     dt, dh);
  QShare qs = {};
  int rc = qshare_pack("jmt_attn_bwd_sq", N, spp, qtab, npair, &qs);
  if (rc != JMT_OK) return rc;
  return attn_bwd_impl(dt, N, H, Lq, Lk, dh, go, sgo_l, sgo_n, o, so_l, so_n, q, sq_l, sq_n, k,
                       sk_l, sk_n, v, sv_l, sv_n, lse, p_out, ds_out, ldp, nullptr, 0, 0, scale,
                       &qs, nullptr, stream);
}

extern "C" int jmt_attn_bwd_sq_kr(int dt, int N, int H, int Lq, int Lk, int dh, const void* go,
                                  int64_t sgo_l, int64_t sgo_n, const void* o, int64_t so_l,
                                  int64_t so_n, const void* q, int64_t sq_l, int64_t sq_n,
                                  const void* k, int64_t sk_l, int64_t sk_n, const void* v,
                                  int64_t sv_l, int64_t sv_n, const float* lse, void* p_out,
                                  void* ds_out, int64_t ldp, float scale, int spp,
                                  const int* qtab, int npair, const int* kr, int kr_mod,
                                  void* stream) {
  if (N == 0 || Lq == 0) return JMT_OK;
  if (!jmt_attn_supported(dt, dh))
    return set_error(JMT_ERR_UNSUPPORTED,
                     "jmt_attn_bwd_sq_kr: dtype %d / head dim %d not supported", dt, dh);
  QShare qs = {};
  int rc = qshare_pack("jmt_attn_bwd_sq_kr", N, spp, qtab, npair, &qs);
  if (rc != JMT_OK) return rc;
  const KeyRange r = {kr, kr_mod};
  return attn_bwd_impl(dt, N, H, Lq, Lk, dh, go, sgo_l, sgo_n, o, so_l, so_n, q, sq_l, sq_n, k,
                       sk_l, sk_n, v, sv_l, sv_n, lse, p_out, ds_out, ldp, nullptr, 0, 0, scale,
                       &qs, &r, stream);
}
