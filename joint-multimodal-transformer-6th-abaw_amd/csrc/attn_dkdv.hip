// Key-side attention gradients from the probabilities the backward kernel hands over (gfx950,
// wave64), head dim 512:
//     dV = P^T dO,   dK = dS^T Q       per (batch n, head h), P / dS [Lq][Lk] from attn_bwd_kernel
// Replaces the two batched TN GEMMs (M = Lk, N = 512, K = Lq, one per product) that ran at
// 250-270 TFLOP/s on the c3 shapes (b384 / b192 x 300 x 512 x 300: profiles/r03_dkdv.jsonl) —
// short contractions whose per-tile prologue and epilogue the generic tile kernel cannot hide.
// Reference: the dK / dV of autograd's backward of F.multi_head_attention_forward behind every
// nn.MultiheadAttention of mm_multi_transformers.py:57,142-167.
//
// Geometry: an item is (n, h, product, 128-key tile) — the product (dV from P and dO, or dK from
// dS and Q) is part of the item, so a block holds one product's 128 x 512 fp32 accumulator (128
// registers per wave) and streams one row operand: per 128 keys it fetches Lq x (1 KiB + 256 B)
// (the two-product 64-key item of the first version fetched Lq x (2 KiB + 256 B) per 64 keys and
// ran at 2.9 TB/s of LDS fill: profiles/r04/dkdv_v1_vs_gemm.jsonl).  Blocks are persistent (one
// per CU, attn.hip's XCD-contiguous item ranges: the key tiles of one head and product share its
// dO / Q rows in one L2) and stream the queries in chunks of 32:
//  * stage = 32 dO / Q rows (1 KiB each, the swizzled row image of attn_common.h) and the P / dS
//    tile of those rows (32 x 128 keys, 256-B rows, 16-B chunk c of row r at c ^ ((r & 7) << 1):
//    conflict-free transposed reads) = 40 KiB; 4 stages (160 KiB), filled by LDS-DMA from inline
//    asm three chunks ahead, across items too; every wait is an exact vmcnt;
//  * wave w owns head dims 64 w .. +63: per chunk one MFMA k-step of 16x16x32 over 8 key groups x
//    4 dim groups.  Both operands come from ds_read_b64_tr_b16 reads (the dims of dO / Q and the
//    keys of P / dS are columns of their images), in the k-slot order of attn.hip's P V product;
//  * queries past Lq (the last chunk) read a clamped row and are zeroed in the P / dS fragment;
//    keys past Lk compute on whatever the P / dS row holds there and are not stored;
//  * the accumulators go straight from registers to HBM (16-B buffer stores of paired subtiles;
//    the buffer range check drops rows past Lk, so every wave issues exactly 16 stores per item
//    and the waits that follow count them).
// HBM bytes per (n, h): Lq rows of dO and of Q (1 KiB each; once per head when its key tiles share
// the L2), Lq x 128 ceil(Lk / 128) x 2 B of P and of dS, Lk rows of dK and of dV written.
//
// Two tiles (template parameter NKG = 16-row groups per item; one instantiation serves the three
// roles of a launch; jmt_attn_dkdv_plan picks per launch):
//  * NKG = 8, the geometry above: 128 rows, 40 KiB stages x 4.
//  * NKG = 10: 160 rows, so L = 300 is two items per product instead of three (6 % padded rows
//    instead of 28 %).  Accumulator 160 registers; the P / dS fragments are read and consumed in
//    two batches of five and the lane bases of the transposed reads are formed by an XOR in front
//    of each read, the row DMA takes a scalar base (glds16_sv): 227 VGPRs, no spills.  The P / dS
//    image is five [32 queries][32 keys] sub-images of 64-B rows (the hand-off's 32-key tiles as
//    they are; chunk c of row r at c ^ 2 in rows 4-7 of every 8: simg_off), the dQ role's dS image
//    160 queries x 32 keys (qimg_off): 42 KiB stages x 3.  Sub-tiles past ldp / 32 (ldp stays
//    128 ceil(Lk / 128): Lk = 130 has 256 columns, the item 320) are clamped to the head's last
//    one; they feed keys past Lk only.  Tile-major P / dS only (dq != NULL).
//  Each output element is contracted over the same 32-deep chunks in the same order by both, so
//  the results are bitwise equal.
//
// Shared queries (template flag SQ, jmt_attn_dkdv_sq): the dK role reads Q through the per-pair
// table of attn_common.h (QShare); with `mrg` the two uses of a query share ONE dQ item whose
// chunk loop runs over the first use's keys and then the second's (dk_decode).  The seam is a
// change of source pointers inside the DMA stream; NDMA per stage and NST per item are unchanged,
// so the accounting below holds as it stands.  SQ = false is the code of before.
//
// vmcnt accounting.  Every wait in the chunk loop is s_waitcnt vmcnt(S NDMA + B NST) with
// immediate operands: S later stages and B items' output stores stay in flight behind the
// awaited stage.  This is exact only if EVERY wave issues the same NDMA DMA wave-instructions per
// stage and the same NST stores per item; a count larger than what a wave really issued
// under-waits (the stage is read before it landed), a smaller one only waits longer.  Hence:
//  * stores are never skipped per wave (the buffer range check drops rows instead): NST = 2 NKG;
//  * the 10 KiB P / dS image of NKG = 10 is ten 1-KiB wave-instructions' worth, which do not deal
//    over 8 waves: each wave issues TWO instructions of 40 active lanes (640 B each; the LDS
//    address is base + 16 lane, so the inactive lanes leave their bytes to the next piece),
//    NDMA = 4 + 2 = 6 for every wave; NKG = 8: 4 + 1 = 5 of 64 lanes;
//  * the largest count, (NS - 2) NDMA + (NS - 1) NST, must fit vmcnt's 6 bits (static_assert).
#include "attn_common.h"

namespace jmt {

constexpr int DK_QC = 32;                               // contraction rows per chunk (one k-step)
constexpr int DK_IMG = DK_QC * AT_ROWB;                 // dO / Q / K row image (32 KiB)
#ifndef JMT_DKDV_NS
#define JMT_DKDV_NS 4                                   // (dev A/B: 3 -> 120 KiB)
#endif

// Tile geometry, NKG = 16-row groups per item: 8 (128 rows) or 10 (160 rows)
template <int NKG>
struct DkGeo {
  static constexpr int KT = 16 * NKG;                   // output rows per item
  static constexpr int PROW = 2 * KT;                   // P / dS image row bytes (128-row form)
  static constexpr int PIMG = DK_QC * PROW;             // P or dS image (8 / 10 KiB)
  static constexpr int STAGE = DK_IMG + PIMG;           // 40 / 42 KiB
  static constexpr int NS = NKG == 8 ? JMT_DKDV_NS : 3; // stages
  static constexpr int LDS = NS * STAGE;                // 160 / 126 KiB
  // the P / dS image is PIMG / 1024 wave-instructions' worth of bytes, dealt as NPD per wave of
  // PLANES active lanes each (8 x 1 x 64 lanes, or 8 x 2 x 40 lanes), so that EVERY wave issues
  // the same NDMA per stage
  static constexpr int NPD = (PIMG / 1024 + 7) / 8;
  static constexpr int PLANES = PIMG / 16 / 8 / NPD;
  static constexpr int NDMA = DK_QC / 8 + NPD;          // DMA wave-instructions per wave per stage
  static constexpr int NST = 2 * NKG;                   // output stores per wave per item
  static_assert(NKG == 8 || NKG == 10, "128- or 160-row items");
  static_assert(NS >= 2 && NS <= 4, "2-4 stages (the wait table covers 0-2 later stages)");
  static_assert(LDS <= 160 * 1024, "stages exceed the LDS");
  static_assert(8 * NPD * PLANES * 16 == PIMG && PLANES <= 64, "P / dS DMA split");
  // the largest count the chunk loop waits on: NS - 2 later stages, NS - 1 items' stores
  static_assert((NS - 2) * NDMA + (NS - 1) * NST < 64, "vmcnt range");
};

struct AttnDkdvArgs {
  const void* p;
  const void* ds;
  const void* go;
  const void* q;
  const void* k;
  void* dk;
  void* dv;
  void* dq;
  int64_t ldp, sgo_l, sgo_n, sq_l, sq_n, sk_l, sk_n, sdk_l, sdk_n, sdv_l, sdv_n, sdq_l, sdq_n;
  int Lq, Lk, H, nkt, nqd, ipn, nitems;
  // jmt_attn_dkdv_sq: the dK role reads the Q of sequence q_seq(qs, n).  With mrg (one dQ per
  // shared query) the items are laid out per group = (first use n1, second use n2, head):
  // n1 = mg_first[u] spp + b, n2 = mg_second[u] spp + b for group (u spp + b) H + h (4-bit fields)
  QShare qs;
  int mrg;
  uint32_t mg_first, mg_second;
};

// byte offset of 16-B chunk `c` of row `r` of the P / dS image of a 128-key item (256-B rows)
__device__ __forceinline__ int pimg_off(int r, int c) {
  return r * DkGeo<8>::PROW + ((c ^ ((r & 7) << 1)) << 4);
}

// byte offset of 16-B chunk `c` of row `r` of one [32 queries][32 keys] sub-image (64-B rows) of
// the P / dS image of a 160-key item (five sub-images, one per 32-key tile of the hand-off):
// chunk c ^ 2 in rows 4-7 of every 8.  A 32-lane half of a ds_read_b64_tr_b16 takes 32 B of each
// of 8 consecutive rows: rows 0-3 and 4-7 then sit in opposite 128-B halves of the 256 B of banks
// (conflict-free); the XOR leaves the order of the two chunks of those 32 B alone.
__device__ __forceinline__ int simg_off(int r, int c) {
  return r * 64 + ((c ^ ((r >> 1) & 2)) << 4);
}

// byte offset of 16-B chunk `c` of row `r` of a dS image of the dQ product (KT query rows x 32
// keys, 64-B rows): chunk c ^ ((r >> 2) & 3), so the two ds_read_b64 of a fragment (rows li of a
// 16-row group, keys 4 g and 16 + 4 g) are conflict-free
__device__ __forceinline__ int qimg_off(int r, int c) {
  return r * 64 + ((c ^ ((r >> 2) & 3)) << 4);
}

// item -> (n H + h, n, h, product (0: dV, 1: dK, 2: dQ), first key (0, 1) or query (2), chunks).
// Per (n, h): nkt dV items, nkt dK items (KT-key tiles, the contraction over queries in 32-row
// chunks), then nqd dQ items (KT-query tiles, the contraction over keys in 32-key chunks).
// Merged dQ (a.mrg): per group the nqd dQ items first (the long ones: they contract over the
// keys of BOTH sequences, nch = 2 nch1, chunks [0, nch1) from n / nh and [nch1, nch) from n2 / nh2,
// each half masked at its own Lk), then the first use's 2 nkt dV / dK items, then the second
// use's.  A group's items are contiguous, so an XCD's range keeps the items that read one head's
// dS together as before, and the long items are spread over the walk, one group apart.
struct DkItem {
  int nh, n, hd, role, k0, nch, nch1, n2, nh2;
};
template <int KT, bool SQ>
__device__ __forceinline__ DkItem dk_decode(const AttnDkdvArgs& a, int it) {
  DkItem d;
  if (SQ && a.mrg) {
    const int gi = it / a.ipn;
    int r = it - gi * a.ipn;
    const int sb = gi / a.H;                            // u spp + b
    d.hd = gi - sb * a.H;
    const int u = sb / a.qs.spp, b = sb - u * a.qs.spp;
    const int n1 = (int)((a.mg_first >> (4 * u)) & 15u) * a.qs.spp + b;
    const int n2 = (int)((a.mg_second >> (4 * u)) & 15u) * a.qs.spp + b;
    if (r < a.nqd) {
      d.role = 2;
      d.k0 = r * KT;
      d.nch1 = (a.Lk + DK_QC - 1) / DK_QC;
      d.nch = 2 * d.nch1;
      d.n = n1;
      d.n2 = n2;
    } else {
      r -= a.nqd;
      const int second = r >= 2 * a.nkt;
      r -= second * 2 * a.nkt;
      d.role = r >= a.nkt;
      d.k0 = (r - d.role * a.nkt) * KT;
      d.nch = d.nch1 = (a.Lq + DK_QC - 1) / DK_QC;
      d.n = d.n2 = second ? n2 : n1;
    }
    d.nh = d.n * a.H + d.hd;
    d.nh2 = d.n2 * a.H + d.hd;
    return d;
  }
  d.nh = it / a.ipn;
  const int r = it - d.nh * a.ipn;
  if (r < 2 * a.nkt) {
    d.role = r >= a.nkt;
    d.k0 = (r - d.role * a.nkt) * KT;
    d.nch = (a.Lq + DK_QC - 1) / DK_QC;
  } else {
    d.role = 2;
    d.k0 = (r - 2 * a.nkt) * KT;
    d.nch = (a.Lk + DK_QC - 1) / DK_QC;
  }
  d.n = d.nh / a.H;
  d.hd = d.nh - d.n * a.H;
  d.nch1 = d.nch;
  d.n2 = d.n;
  d.nh2 = d.nh;
  return d;
}

// one stage of a 128-row item: rows q0 .. q0+31 (clamped to Lq - 1) of dO or Q, and of the P or dS
// tile (keys k0 .. k0+127): 4 + 1 DMA wave-instructions per wave.  Row offsets in 32-bit byte
// arithmetic from a per-head base (the host checks Lq rows fit): the 64-bit row products of
// stage_rows cost ~25 scalar instructions per DMA, and the CU's one scalar unit serves all 8 waves.
// `c` is the item's chunk: contraction rows 32 c .. +31, or for the second half of a merged dQ
// item (c >= nch1) keys 32 (c - nch1) .. +31 of the second use's sequence.
template <typename T, bool SQ>
__device__ __forceinline__ void dkdv_stage(char* st, const AttnDkdvArgs& a, const DkItem& d,
                                           int c) {
  const int lane = threadIdx.x & 63;
  const int wu = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool second = SQ && c >= d.nch1;                // merged dQ items only
  const int q0 = DK_QC * (second ? c - d.nch1 : c);
  if (d.role == 2) {
    const int sn = second ? d.n2 : d.n, snh = second ? d.nh2 : d.nh;
    // dQ chunk: K rows q0 .. q0+31 (here q0 is the first KEY of the chunk) and the dS tile of the
    // item's 128 queries x those 32 keys (one wave-instruction per wave: 16 rows of 64 B)
    const char* kb = (const char*)((const T*)a.k + (int64_t)sn * a.sk_n + d.hd * AT_DH);
    const int ldk = (int)(a.sk_l * (int64_t)sizeof(T));
#pragma unroll
    for (int i = 0; i < DK_QC / 8; ++i) {
      const int r = wu * (DK_QC / 8) + i;
      const int src = min(q0 + r, a.Lk - 1);
      const unsigned off = (unsigned)(lane ^ ((r & 7) << 1)) << 4;
      glds16_asm(kb + (unsigned)(src * ldk) + off, st + r * AT_ROWB);
    }
    const int r = 16 * wu + (lane >> 2);                // dS image row (query d.k0 + r)
    const int lc = (lane & 3) ^ ((r >> 2) & 3);         // the logical chunk this lane's 16 B hold
    const int src_row = min(d.k0 + r, a.Lq - 1);
    JMT_DCHECK(src_row >= 0 && q0 + 8 * lc + 8 <= a.ldp);
    // tile-major dS (jmt_attn_bwd with dq = NULL): [key tile q0 / 32][query][32 keys]
    const char* pb = (const char*)((const T*)a.ds + (int64_t)snh * a.Lq * a.ldp);
    glds16_asm(pb + (unsigned)(((q0 >> 5) * a.Lq + src_row) * 64) + 16 * lc,
               st + DK_IMG + wu * 1024);
    return;
  }
  const char* rb;
  int ldb;
  if (d.role == 0) {
    rb = (const char*)((const T*)a.go + (int64_t)d.n * a.sgo_n + d.hd * AT_DH);
    ldb = (int)(a.sgo_l * (int64_t)sizeof(T));
  } else {
    rb = (const char*)((const T*)a.q + (int64_t)q_seq<SQ>(a.qs, d.n) * a.sq_n + d.hd * AT_DH);
    ldb = (int)(a.sq_l * (int64_t)sizeof(T));
  }
#pragma unroll
  for (int i = 0; i < DK_QC / 8; ++i) {
    const int r = wu * (DK_QC / 8) + i;
    const int src = min(q0 + r, a.Lq - 1);
    const unsigned off = (unsigned)(lane ^ ((r & 7) << 1)) << 4;
    glds16_asm(rb + (unsigned)(src * ldb) + off, st + r * AT_ROWB);
  }
  const int r = 4 * wu + (lane >> 4);                   // P / dS image row of this lane's 16 B
  const int cs = (lane & 15) ^ ((r & 7) << 1);          // the logical chunk it holds
  const int src_row = min(q0 + r, a.Lq - 1);
  JMT_DCHECK(src_row >= 0 && d.k0 + 8 * cs + 8 <= a.ldp);
  if (a.dq) {      // tile-major P / dS (jmt_attn_bwd with dq = NULL): [key tile][query][32 keys]
    const char* pb = (const char*)((const T*)(d.role == 0 ? a.p : a.ds) +
                                   (int64_t)d.nh * a.Lq * a.ldp);
    glds16_asm(pb + (unsigned)((((d.k0 >> 5) + (cs >> 2)) * a.Lq + src_row) * 64) +
                   16 * (cs & 3),
               st + DK_IMG + wu * 1024);
    return;
  }
  const char* pb = (const char*)((const T*)(d.role == 0 ? a.p : a.ds) +
                                 (int64_t)d.nh * a.Lq * a.ldp + d.k0);
  glds16_asm(pb + (unsigned)(src_row * (int)(a.ldp * sizeof(T))) + 16 * cs,
             st + DK_IMG + wu * 1024);
}

// one stage of a 160-row item (tile-major P / dS only): the 32 rows as above (scalar row base +
// lane offset), and the 10 KiB P / dS image as two wave-instructions of 40 active lanes per wave
// (wave w, instruction j: image bytes 640 (2 w + j) .. +639).  dV / dK: five [32 queries][32 keys]
// sub-images (simg_off), sub-image s from hand-off tile k0 / 32 + s, clamped to the last tile of
// the head's region (ldp / 32 - 1: ldp covers 128-key tiles only, and the tile after belongs to
// the next head; a clamped tile feeds keys past Lk, which are not stored).  dQ: 160 queries x the
// chunk's 32 keys (qimg_off), from hand-off tile q0 / 32.
template <typename T, bool SQ>
__device__ __forceinline__ void dkdv_stage160(uint32_t st, const AttnDkdvArgs& a, const DkItem& d,
                                              int ch) {
  typedef DkGeo<10> G;
  const int lane = threadIdx.x & 63;
  const int wu = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool second = SQ && ch >= d.nch1;               // merged dQ items only (as dkdv_stage)
  const int q0 = DK_QC * (second ? ch - d.nch1 : ch);
  const int snh = second ? d.nh2 : d.nh;
  const char* rb;
  int ldb, clen;
  if (d.role == 0) {
    rb = (const char*)((const T*)a.go + (int64_t)d.n * a.sgo_n + d.hd * AT_DH);
    ldb = (int)(a.sgo_l * (int64_t)sizeof(T));
    clen = a.Lq;
  } else if (d.role == 1) {
    rb = (const char*)((const T*)a.q + (int64_t)q_seq<SQ>(a.qs, d.n) * a.sq_n + d.hd * AT_DH);
    ldb = (int)(a.sq_l * (int64_t)sizeof(T));
    clen = a.Lq;
  } else {
    rb = (const char*)((const T*)a.k + (int64_t)(second ? d.n2 : d.n) * a.sk_n + d.hd * AT_DH);
    ldb = (int)(a.sk_l * (int64_t)sizeof(T));
    clen = a.Lk;
  }
#pragma unroll
  for (int i = 0; i < DK_QC / 8; ++i) {
    const int r = wu * (DK_QC / 8) + i;
    const int src = min(q0 + r, clen - 1);
    JMT_DCHECK(src >= 0 && src < clen);
    const unsigned off = (unsigned)(lane ^ ((r & 7) << 1)) << 4;
    glds16_sv(rb + (unsigned)(src * ldb), off, st + r * AT_ROWB);
  }
  const char* pb = (const char*)((const T*)(d.role == 0 ? a.p : a.ds) +
                                 (int64_t)snh * a.Lq * a.ldp);
  const int ntile = (int)(a.ldp >> 5);                  // 32-key tiles of the head's region
  if (lane < G::PLANES) {
#pragma unroll
    for (int j = 0; j < G::NPD; ++j) {
      const int b0 = (wu * G::NPD + j) * (16 * G::PLANES);
      const int b = b0 + 16 * lane;                     // image byte of this lane's 16 B
      const int pc = (b >> 4) & 3;                      // physical chunk of its 64-B row
      int tile, row, c;
      if (d.role == 2) {
        const int r = b >> 6;                           // dS image row (query d.k0 + r)
        c = pc ^ ((r >> 2) & 3);
        tile = q0 >> 5;
        row = min(d.k0 + r, a.Lq - 1);
      } else {
        const int r = (b >> 6) & 31;                    // sub-image row (query q0 + r)
        c = pc ^ ((r >> 1) & 2);
        tile = min((d.k0 >> 5) + (b >> 11), ntile - 1);
        row = min(q0 + r, a.Lq - 1);
      }
      JMT_DCHECK(row >= 0 && tile >= 0 && tile < ntile);
      glds16_sv(pb, (unsigned)((tile * a.Lq + row) * 64 + 16 * c), st + DK_IMG + b0);
    }
  }
}

// s_waitcnt vmcnt(stages * NDMA + stores * NST) for the counts the chunk loop meets: 0 .. NS - 2
// later stages and 0 .. NS - 1 items' output stores in flight behind the awaited stage
template <int NKG, int S>
__device__ __forceinline__ void dkdv_wait_s(int stores) {
  typedef DkGeo<NKG> G;
  if constexpr (S <= G::NS - 2) {
    if (stores == 0) wait_vmcnt<S * G::NDMA>();
    else if (stores == 1 || G::NS == 2) wait_vmcnt<S * G::NDMA + G::NST>();
    else if constexpr (G::NS >= 3) {
      if (stores == 2 || G::NS == 3) wait_vmcnt<S * G::NDMA + 2 * G::NST>();
      else if constexpr (G::NS >= 4) wait_vmcnt<S * G::NDMA + 3 * G::NST>();
    }
  } else {
    wait_vmcnt<0>();
  }
}
template <int NKG>
__device__ __forceinline__ void dkdv_wait(int stages, int stores) {
  if (stages == 0) dkdv_wait_s<NKG, 0>(stores);
  else if (stages == 1) dkdv_wait_s<NKG, 1>(stores);
  else dkdv_wait_s<NKG, 2>(stores);
}

// Between the dS fragment reads of the dQ role: keeps hipcc from pairing two ds_read_b64 (rows 16
// apart, or the two key halves) into one ds_read2st64_b64, which banks modulo 32 dwords and takes
// 16 LDS cycles for what two ds_read_b64 do in 4: SQ_LDS_BANK_CONFLICT 27 % of SQ_LDS_IDX_ACTIVE
// with the paired reads, 0 without, and 40 % fewer active LDS cycles (profiles/r09/dkdv_pmc*.txt).
#define DK_NO_MERGE() asm volatile("" ::: "memory")

template <typename T, int NKG, bool SQ>
__global__ __launch_bounds__(512, 2) void attn_dkdv_kernel(AttnDkdvArgs a) {
  typedef typename Frag16<T>::t F;
  typedef typename Frag16<T>::h Hf;
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  typedef DkGeo<NKG> G;
  constexpr int KT = G::KT, NS = G::NS, STAGE = G::STAGE;
  constexpr int KB = NKG == 8 ? 8 : 5;                  // P / dS fragments read per batch
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int g = lane >> 4, li = lane & 15;
  int item, iend, istride;
  item_range(a.nitems, item, iend, istride);
  if (item >= iend) return;

  // transposed-read lane bases.  128 rows: one register per read, tb[t] and pb[kg].  160 rows:
  // tb[t] = tb[0] ^ (t << 5) (the swizzle XOR and t sit in the same chunk bits) and the P / dS
  // read of key group kg at (pb[0] ^ ((kg & 1) << 5)) + 2048 (kg >> 1), formed in front of the
  // reads: the accumulator leaves no registers for 12 bases.
  int tb[NKG == 8 ? 4 : 1], pb[NKG == 8 ? 8 : 1];
  if constexpr (NKG == 8) {
#pragma unroll
    for (int t = 0; t < 4; ++t) tb[t] = tr_base(4 * (w & 1) + t, li, g, 0) + 256 * (w >> 1);
#pragma unroll
    for (int kg = 0; kg < 8; ++kg)
      pb[kg] = pimg_off(4 * g + (li >> 2), 2 * kg + ((li & 3) >> 1)) + 8 * (li & 1);
  } else {
    tb[0] = tr_base(4 * (w & 1), li, g, 0) + 256 * (w >> 1);
    pb[0] = simg_off(4 * g + (li >> 2), (li & 3) >> 1) + 8 * (li & 1);
  }
  auto lane_base = [](int base, int bits) __attribute__((always_inline)) {
#if !defined(__OPTIMIZE__)
    return base ^ bits;
#else
    int r;
    asm volatile("v_xor_b32 %0, %2, %1" : "=v"(r) : "v"(base), "i"(bits));
    return r;
#endif
  };
  // dQ: dS fragment of query group qg = rows 16 qg + li, keys 4 g .. +3 (k-slots 0-3) and
  // 16 + 4 g .. +3 (k-slots 4-7): the k-slot order of the transposed K-row reads
  const int qb0 = qimg_off(li, g >> 1) + 8 * (g & 1);
  const int qb1 = NKG == 8 ? qimg_off(li, 2 + (g >> 1)) + 8 * (g & 1) : 0;   // 160: qb0 ^ 32
  const uint32_t lbase = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;

  // issue cursor: the chunk whose stage goes out next (runs NS - 1 chunks ahead of the compute)
  int is_item = item, is_c = 0;
  DkItem is_d = dk_decode<KT, SQ>(a, item);
  bool is_ok = true;
  int is_buf = 0;
  unsigned after = 0;      // 4 bits per buffer: store batches issued after the stage it holds
  int inflight = 0;        // stages issued and not yet waited for
  auto issue = [&]() {
    if (is_ok) {
      if constexpr (NKG == 8) dkdv_stage<T, SQ>(smem + is_buf * STAGE, a, is_d, is_c);
      else dkdv_stage160<T, SQ>(lbase + is_buf * STAGE, a, is_d, is_c);
      after &= ~(15u << (4 * is_buf));
      ++inflight;
      if (++is_c == is_d.nch) {
        is_c = 0;
        is_item += istride;
        is_ok = is_item < iend;
        if (is_ok) is_d = dk_decode<KT, SQ>(a, is_item);
      }
    }
    is_buf = is_buf == NS - 1 ? 0 : is_buf + 1;
  };
  for (int i = 0; i < NS - 1; ++i) issue();
  int buf = 0;

  while (true) {
    const DkItem d = dk_decode<KT, SQ>(a, item);
    const bool more = item + istride < iend;
    f32x4 acc[NKG][4];
#pragma unroll
    for (int kg = 0; kg < NKG; ++kg)
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[kg][t] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int c = 0; c < d.nch; ++c) {
      const char* cur = smem + buf * STAGE;
      // this chunk's stage landed (the later stages and the output stores issued after it may
      // stay in flight), and every wave is done reading the buffer restaged below
      dkdv_wait<NKG>(inflight - 1, (after >> (4 * buf)) & 15);
      --inflight;
      lds_barrier();
      issue();
      // first contraction index of the chunk (a merged dQ item: within its half's keys, so the
      // last chunk of EACH sequence's key range is masked)
      const int c0 = DK_QC * (SQ && c >= d.nch1 ? c - d.nch1 : c);
      const int clen = d.role == 2 ? a.Lk : a.Lq;       // contraction length
      F df[4];
      // the P / dS fragments in batches of KB groups (128 rows: one batch, read before the dO /
      // Q / K fragments; 160 rows: two of five, 20 registers live instead of 40)
#pragma unroll
      for (int k0 = 0; k0 < NKG; k0 += KB) {
        F kf[KB];
        if (d.role != 2) {
#pragma unroll
          for (int j = 0; j < KB; ++j) {
            const int kg = k0 + j;
            const char* pa;
            if constexpr (NKG == 8) pa = cur + DK_IMG + pb[kg];
            else pa = cur + DK_IMG + lane_base(pb[0], (kg & 1) << 5) + 2048 * (kg >> 1);
            const Hf lo = tr_read<Hf>(pa);
            const Hf hi = tr_read<Hf>(pa + (NKG == 8 ? 16 * G::PROW : 16 * 64));
            kf[j] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
          }
        } else {
          const char* qa0 = cur + DK_IMG + qb0;
          const char* qa1;
          if constexpr (NKG == 8) qa1 = cur + DK_IMG + qb1;
          else qa1 = cur + DK_IMG + lane_base(qb0, 32);
#pragma unroll
          for (int j = 0; j < KB; ++j) {
            const Hf lo = *(const Hf*)(qa0 + 1024 * (k0 + j));
            DK_NO_MERGE();
            const Hf hi = *(const Hf*)(qa1 + 1024 * (k0 + j));
            DK_NO_MERGE();
            kf[j] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
          }
        }
        // k-slot e holds contraction index c0 + 16 (e >> 2) + 4 g + (e & 3)
        if (c0 + DK_QC > clen) {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const bool in = c0 + 16 * (e >> 2) + 4 * g + (e & 3) < clen;
#pragma unroll
            for (int j = 0; j < KB; ++j) kf[j][e] = in ? kf[j][e] : from_f<T>(0.f);
          }
        }
        if (k0 == 0) {
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const char* ta;
            if constexpr (NKG == 8) ta = cur + tb[t];
            else ta = cur + lane_base(tb[0], t << 5);
            const Hf lo = tr_read<Hf>(ta);
            const Hf hi = tr_read<Hf>(ta + 16 * AT_ROWB);
            df[t] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
          }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int j = 0; j < KB; ++j) acc[k0 + j][t] = mfma16(df[t], kf[j], acc[k0 + j][t]);
      }
      buf = buf == NS - 1 ? 0 : buf + 1;
    }

    // ---- outputs: lane = key (dQ: query) k0 + 16 kg + li, dims 64 w + 16 t + 4 g + r; subtiles
    // t, t + 1 paired by v_permlane16_swap into 8 consecutive dims per lane (store_acc_direct's
    // scheme)
    {
      T* ob = d.role == 0 ? (T*)a.dv + (int64_t)d.n * a.sdv_n
            : d.role == 1 ? (T*)a.dk + (int64_t)d.n * a.sdk_n : (T*)a.dq + (int64_t)d.n * a.sdq_n;
      const int64_t sl = d.role == 0 ? a.sdv_l : d.role == 1 ? a.sdk_l : a.sdq_l;
      ob += (int64_t)d.hd * AT_DH + (int64_t)d.k0 * sl;
      const uint64_t ba = (uint64_t)(uintptr_t)ob;
      const uint32_t blo = __builtin_amdgcn_readfirstlane((uint32_t)ba);
      const uint32_t bhi = __builtin_amdgcn_readfirstlane((uint32_t)(ba >> 32));
      const int nrows = min(KT, (d.role == 2 ? a.Lq : a.Lk) - d.k0);
      const int bytes = __builtin_amdgcn_readfirstlane((int)(nrows * sl * (int64_t)sizeof(T)));
      const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(((uint64_t)bhi << 32) | blo), 0, bytes, 0x00020000);
      const int sl32 = (int)sl;
#pragma unroll
      for (int kg = 0; kg < NKG; ++kg) {
#pragma unroll
        for (int jp = 0; jp < 2; ++jp) {
          uint32_t pk[2][2];
#pragma unroll
          for (int hh = 0; hh < 2; ++hh)
#pragma unroll
            for (int qq = 0; qq < 2; ++qq) {
              T two[2] = {from_f<T>(acc[kg][2 * jp + hh][2 * qq]),
                          from_f<T>(acc[kg][2 * jp + hh][2 * qq + 1])};
              pk[hh][qq] = *(const uint32_t*)two;
            }
          const auto r0 = __builtin_amdgcn_permlane16_swap(pk[0][0], pk[1][0], false, false);
          const auto r1 = __builtin_amdgcn_permlane16_swap(pk[0][1], pk[1][1], false, false);
          const int col = 64 * w + 16 * (2 * jp + (g & 1)) + 8 * (g >> 1);
          const u32x4 v = {r0[0], r1[0], r0[1], r1[1]};
          const int off = ((16 * kg + li) * sl32 + col) * (int)sizeof(T);
          __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, off, 0, 0);
        }
      }
    }
    // these stores follow the stages in flight (the next chunks'; the free buffer's count is
    // reset when it is restaged)
    after += 0x1111;
    if (!more) break;
    item += istride;
  }
  wait_vmcnt<0>();
}

static int dkdv_grid(int nitems) {
  static int ncu = 0;
  if (ncu == 0) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v < 8)
      v = 8;
    ncu = v / 8 * 8;
  }
  return nitems > ncu ? ncu : nitems;
}

// ---- which tile a launch takes
// Cost of a head with KT-row items: 2 ceil(Lk / KT) dV / dK items of ceil(Lq / 32) chunks and
// ceil(Lq / KT) dQ items of ceil(Lk / 32) chunks, a chunk priced at the item's KT rows.  The
// bytes staged per chunk (32 KiB + 64 KT B) grow by 5 % from 128 to 160 rows, but the measured
// time per chunk grows with the rows (x 1.24-1.29 for x 1.25: profiles/r09/dkdv_tiles.txt), so a
// launch gains what the larger tile saves in padded rows and loses where it pads more
// (L = 1024: 1120 rows against 1024, +9 % measured).
static int64_t dkdv_cost(int Lq, int Lk, int KT) {
  const auto cdiv = [](int x, int d) { return ((int64_t)x + d - 1) / d; };
  return (2 * cdiv(Lk, KT) * cdiv(Lq, DK_QC) + cdiv(Lq, KT) * cdiv(Lk, DK_QC)) * KT;
}

// JMT_ATTN_DKDV_KT = 0 (the rule) / 128 / 160, read once; jmt_attn_dkdv_set_tile overrides it
// in-process (tests and scripts/bench_dkdv.py compare the two tiles), -1 returns to the
// environment's choice
static int g_dkdv_tile = -1;
static int dkdv_tile_pref() {
  static const int env = [] {
    const char* e = getenv("JMT_ATTN_DKDV_KT");
    const int v = e ? atoi(e) : 0;
    return v == 128 || v == 160 ? v : 0;
  }();
  return g_dkdv_tile < 0 ? env : g_dkdv_tile;
}

static int dkdv_plan(int Lq, int Lk, int64_t sdk_l, int64_t sdv_l, int64_t sdq_l, bool has_dq) {
  constexpr int64_t KT = DkGeo<10>::KT;
  // 160-row items read the tile-major hand-off only (dq != NULL) and need their 32-bit store
  // offsets to cover 160 rows; where they do not, the launch is a valid 128-row one
  if (!has_dq || Lq <= 0 || Lk <= 0 || KT * sdk_l * 2 >= (1LL << 31) ||
      KT * sdv_l * 2 >= (1LL << 31) || KT * sdq_l * 2 >= (1LL << 31))
    return 128;
  const int pref = dkdv_tile_pref();
  if (pref) return pref;
  return dkdv_cost(Lq, Lk, 160) < dkdv_cost(Lq, Lk, 128) ? 160 : 128;   // ties keep 128
}

// nullptr when jmt_attn_dkdv takes these sizes and row strides (host only, no pointer: the entry
// point validates with it and jmt_attn_dkdv_ok answers from it), else what is out of range.
// sk_l / sdq_l count with has_dq only.
static const char* dkdv_range(int N, int H, int Lq, int Lk, int64_t ldp, int64_t sgo_l,
                              int64_t sq_l, int64_t sk_l, int64_t sdk_l, int64_t sdv_l,
                              int64_t sdq_l, bool has_dq) {
  constexpr int64_t DK_KT = DkGeo<8>::KT;              // the contract's tile: ldp, stride ranges
  constexpr int64_t LIM = 1LL << 31;                   // 32-bit byte offsets of 16-bit elements
  if (!(N > 0 && H > 0 && Lq > 0 && Lk > 0)) return "bad sizes";
  if (ldp < (Lk + DK_KT - 1) / DK_KT * DK_KT) return "ldp must cover 128-key tiles";
  if (sdk_l < H * AT_DH || sdv_l < H * AT_DH || DK_KT * sdk_l * 2 >= LIM ||
      DK_KT * sdv_l * 2 >= LIM)
    return "dK / dV row stride out of range";
  if (has_dq) {
    if (sdq_l < H * AT_DH || DK_KT * sdq_l * 2 >= LIM || Lk * sk_l * 2 >= LIM)
      return "dQ / K row stride out of range";
    // the tile-major region of head nh starts at nh Lq ldp: whole 32-key tiles only
    if (ldp % 32 != 0) return "tile-major P / dS need ldp % 32 == 0";
  }
  const int kt = dkdv_plan(Lq, Lk, sdk_l, sdv_l, has_dq ? sdq_l : 0, has_dq);
  const int nkt = (Lk + kt - 1) / kt;
  const int nqd = has_dq ? (Lq + kt - 1) / kt : 0;     // dQ items per (n, h)
  if ((int64_t)N * H * (2 * nkt + nqd) >= LIM) return "too many items";
  if (Lq * sgo_l * 2 >= LIM || Lq * sq_l * 2 >= LIM || Lq * ldp * 2 >= LIM)
    return "Lq rows of dO / Q / P exceed 2 GiB";
  return nullptr;
}

template <typename T, int NKG, bool SQ>
static void dkdv_launch_sq(const AttnDkdvArgs& a, int grid, hipStream_t st) {
  constexpr int lds = DkGeo<NKG>::LDS;
  static bool once = ((void)hipFuncSetAttribute((const void*)attn_dkdv_kernel<T, NKG, SQ>,
                                                hipFuncAttributeMaxDynamicSharedMemorySize, lds),
                      true);
  (void)once;
  hipLaunchKernelGGL((attn_dkdv_kernel<T, NKG, SQ>), dim3(grid), dim3(512), (size_t)lds, st, a);
}
template <typename T, int NKG>
static void dkdv_launch(const AttnDkdvArgs& a, int grid, hipStream_t st, bool sq) {
  if (sq) dkdv_launch_sq<T, NKG, true>(a, grid, st);
  else dkdv_launch_sq<T, NKG, false>(a, grid, st);
}

}  // namespace jmt

using namespace jmt;

extern "C" int jmt_attn_dkdv_set_tile(int kt) {
  if (!(kt < 0 || kt == 0 || kt == 128 || kt == 160))
    return set_error(JMT_ERR_ARG, "jmt_attn_dkdv_set_tile: %d is not 0, 128 or 160", kt);
  g_dkdv_tile = kt < 0 ? -1 : kt;
  return JMT_OK;
}

extern "C" int jmt_attn_dkdv_plan(int Lq, int Lk, int H, int64_t sdk_l, int64_t sdv_l,
                                  int64_t sdq_l, int has_dq) {
  (void)H;
  return dkdv_plan(Lq, Lk, sdk_l, sdv_l, sdq_l, has_dq != 0);
}

extern "C" int jmt_attn_dkdv_ok(int N, int H, int Lq, int Lk, int64_t ldp, int64_t sgo_l,
                                int64_t sq_l, int64_t sk_l, int64_t sdk_l, int64_t sdv_l,
                                int64_t sdq_l, int has_dq) {
  return dkdv_range(N, H, Lq, Lk, ldp, sgo_l, sq_l, sk_l, sdk_l, sdv_l, sdq_l, has_dq != 0) ==
         nullptr;
}

// jmt_attn_dkdv (qs == NULL) and jmt_attn_dkdv_sq (qs: the packed query table of npair pairs;
// merge: one dQ per shared query, qtab the table qs was packed from)
static int dkdv_impl(int dt, int N, int H, int Lq, int Lk, int dh, const void* p, const void* ds,
                     int64_t ldp, const void* go, int64_t sgo_l, int64_t sgo_n, const void* q,
                     int64_t sq_l, int64_t sq_n, const void* k, int64_t sk_l, int64_t sk_n,
                     void* dk, int64_t sdk_l, int64_t sdk_n, void* dv, int64_t sdv_l,
                     int64_t sdv_n, void* dq, int64_t sdq_l, int64_t sdq_n, const QShare* qs,
                     const int* qtab, int npair, int merge, void* stream) {
  if (N == 0 || Lk == 0) return JMT_OK;
  if (!((dt == JMT_BF16 || dt == JMT_F16) && dh == AT_DH))
    return set_error(JMT_ERR_UNSUPPORTED, "jmt_attn_dkdv: dtype %d / head dim %d not supported",
                     dt, dh);
  const void* ptrs[] = {p, ds, go, q, dk, dv};
  for (int i = 0; i < 6; ++i)
    JMT_CHECK_ARG(ptrs[i] != nullptr && ((uintptr_t)ptrs[i] & 15) == 0,
                  "jmt_attn_dkdv: operand %d null or not 16-B aligned", i);
  const int64_t strides[] = {ldp, sgo_l, sgo_n, sq_l, sq_n, sdk_l, sdk_n, sdv_l, sdv_n};
  for (int i = 0; i < 9; ++i)
    JMT_CHECK_ARG(strides[i] % 8 == 0, "jmt_attn_dkdv: stride %d not a multiple of 8", i);
  if (dq)
    JMT_CHECK_ARG(k != nullptr && ((uintptr_t)k & 15) == 0 && ((uintptr_t)dq & 15) == 0 &&
                      sk_l % 8 == 0 && sk_n % 8 == 0 && sdq_l % 8 == 0 && sdq_n % 8 == 0,
                  "jmt_attn_dkdv: k / dq null, misaligned or strides not multiples of 8");
  const char* why = dkdv_range(N, H, Lq, Lk, ldp, sgo_l, sq_l, sk_l, sdk_l, sdv_l, sdq_l,
                               dq != nullptr);
  JMT_CHECK_ARG(!why, "jmt_attn_dkdv: %s", why);
  const int kt = dkdv_plan(Lq, Lk, sdk_l, sdv_l, dq ? sdq_l : 0, dq != nullptr);
  const int nkt = (Lk + kt - 1) / kt;
  const int nqd = dq ? (Lq + kt - 1) / kt : 0;          // dQ items per (n, h)
  AttnDkdvArgs a = {};
  if (qs) a.qs = *qs;
  a.p = p; a.ds = ds; a.go = go; a.q = q; a.k = k; a.dk = dk; a.dv = dv; a.dq = dq;
  a.ldp = ldp; a.sgo_l = sgo_l; a.sgo_n = sgo_n; a.sq_l = sq_l; a.sq_n = sq_n;
  a.sk_l = sk_l; a.sk_n = sk_n;
  a.sdk_l = sdk_l; a.sdk_n = sdk_n; a.sdv_l = sdv_l; a.sdv_n = sdv_n;
  a.sdq_l = sdq_l; a.sdq_n = sdq_n;
  a.Lq = Lq; a.Lk = Lk; a.H = H; a.nkt = nkt; a.nqd = nqd; a.ipn = 2 * nkt + nqd;
  a.nitems = N * H * a.ipn;
  if (merge) {
    // every pair is a first use with exactly one second use, or that second use: npair / 2
    // groups of nqd merged dQ items + the two sequences' dV / dK items
    int ng = 0;
    for (int f = 0; f < npair; ++f) {
      if (qtab[f] != f) continue;
      int second = -1, uses = 0;
      for (int j = 0; j < npair; ++j)
        if (j != f && qtab[j] == f) { second = j; ++uses; }
      if (uses != 1)
        return set_error(JMT_ERR_UNSUPPORTED, "jmt_attn_dkdv_sq: merged dQ needs every query "
                                              "used exactly twice (pair %d: %d more uses)",
                         f, uses);
      a.mg_first |= (uint32_t)f << (4 * ng);
      a.mg_second |= (uint32_t)second << (4 * ng);
      ++ng;
    }
    a.mrg = 1;
    a.ipn = nqd + 4 * nkt;
    a.nitems = ng * a.qs.spp * H * a.ipn;
  }
  const int grid = dkdv_grid(a.nitems);
  hipStream_t st = as_stream(stream);
  if (kt == 160) {
    if (dt == JMT_BF16) dkdv_launch<__bf16, 10>(a, grid, st, qs != nullptr);
    else dkdv_launch<_Float16, 10>(a, grid, st, qs != nullptr);
  } else {
    if (dt == JMT_BF16) dkdv_launch<__bf16, 8>(a, grid, st, qs != nullptr);
    else dkdv_launch<_Float16, 8>(a, grid, st, qs != nullptr);
  }
  JMT_LAUNCH_CHECK("jmt_attn_dkdv");
  return JMT_OK;
}

extern "C" int jmt_attn_dkdv(int dt, int N, int H, int Lq, int Lk, int dh, const void* p,
                             const void* ds, int64_t ldp, const void* go, int64_t sgo_l,
                             int64_t sgo_n, const void* q, int64_t sq_l, int64_t sq_n,
                             const void* k, int64_t sk_l, int64_t sk_n, void* dk, int64_t sdk_l,
                             int64_t sdk_n, void* dv, int64_t sdv_l, int64_t sdv_n, void* dq,
                             int64_t sdq_l, int64_t sdq_n, void* stream) {
  return dkdv_impl(dt, N, H, Lq, Lk, dh, p, ds, ldp, go, sgo_l, sgo_n, q, sq_l, sq_n, k, sk_l,
                   sk_n, dk, sdk_l, sdk_n, dv, sdv_l, sdv_n, dq, sdq_l, sdq_n, nullptr, nullptr,
                   0, 0, stream);
}

extern "C" int jmt_attn_dkdv_sq(int dt, int N, int H, int Lq, int Lk, int dh, const void* p,
                                const void* ds, int64_t ldp, const void* go, int64_t sgo_l,
                                int64_t sgo_n, const void* q, int64_t sq_l, int64_t sq_n,
                                const void* k, int64_t sk_l, int64_t sk_n, void* dk,
                                int64_t sdk_l, int64_t sdk_n, void* dv, int64_t sdv_l,
                                int64_t sdv_n, void* dq, int64_t sdq_l, int64_t sdq_n, int spp,
                                const int* qtab, int npair, int merge_dq, void* stream) {
  if (N == 0 || Lk == 0) return JMT_OK;
  if (!((dt == JMT_BF16 || dt == JMT_F16) && dh == AT_DH))
    return set_error(JMT_ERR_UNSUPPORTED,
                     "jmt_attn_dkdv_sq: dtype %d / head dim %d not supported", dt, dh);
  if (dq == nullptr)
    return set_error(JMT_ERR_UNSUPPORTED, "jmt_attn_dkdv_sq: the tile-major form only (dq != "
                                          "NULL: P / dS from jmt_attn_bwd_sq)");
  QShare qs = {};
  int rc = qshare_pack("jmt_attn_dkdv_sq", N, spp, qtab, npair, &qs);
  if (rc != JMT_OK) return rc;
  return dkdv_impl(dt, N, H, Lq, Lk, dh, p, ds, ldp, go, sgo_l, sgo_n, q, sq_l, sq_n, k, sk_l,
                   sk_n, dk, sdk_l, sdk_n, dv, sdv_l, sdv_n, dq, sdq_l, sdq_n, &qs, qtab, npair,
                   merge_dq != 0, stream);
}
