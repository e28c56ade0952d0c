// conv_igemm.h — MFMA implicit-GEMM 3x3/1x1 convolution for gfx950 with the LRP epilogues fused.  This one kernel
// family carries >95 % of the FLOPs of the hot path:
//   * encoder forward: the dual conv a_l | Z+_l (EPI_FWD_DUAL: fp16 pairs, TERMS 7 / 23, or exact fp32), the activation
//     chain (EPI_BIAS_RELU) and denominators Z+ (EPI_BIAS) in split-bf16 (TERMS 7)          — per image, cached
//   * conv-LRP alpha1beta0 backward (EPI_MUL / EPI_MUL_UP2 / EPI_IMG_STENCIL)              — per token
//     RR:274-322 restructured: S_{l-1} = up2?(convT(S_l, w_l+)) * G_{l-1}
//     alpha-beta with beta > 0: both chains [S+ | S-] through one GEMM against [alpha w+ ; -beta w-], two gates on one
//     accumulator (template DG, ConvArgs::aux_b)                                          — per token, lrp_set_cnn_rule
//   * every dense product of the decoder LRP / gradient paths (taps = 1, EPI_STORE / EPI_MUL)
// Template axes: tile (WM, WN, TM, TN), epilogue EPI, operand arithmetic PREC (exact fp32 MFMA | split-bf16),
// HALO (3x3: A tile + halo resident in LDS for all 9 taps), BREG (weights in registers, no barrier per tap: N <= 64, and the 8-wave tile),
// TERMS (which partial products of the split operands are issued).  DESIGN.md 4.1 has the measurements behind each.
// This file is the kernel alone: its arguments are conv_args.h, its tile constants (ConvKernelTraits) and the pieces of its body
// that stand on their own conv_tile.h, which instantiations exist and which one a launch takes is conv_plan.h, the launchers are
// conv_launch.h.  A translation unit that wants ONE instantiation (ISA inspection) includes this file.
//
// GEMM view: D[m][n] = sum_k A[m][k] * B[k][n],  m = output pixel (NHWC row),
// n = output channel, k = (tap, input channel).  A is gathered on the fly
// (im2col never materialised); B is pre-packed [n][k] so both operands are
// "rows of 32 consecutive k" = 128 B, staged through LDS unpadded with an XOR
// swizzle of the 16 B chunk index, chunk ^ ((row>>1)&7): conflict-free for the
// ds_read_b128 fragment reads AND the ds_write_b128 staging writes.
//
// MFMA: v_mfma_f32_32x32x2_f32 (exact fp32, 64 FLOP/clk/SIMD).  Lane l feeds
// A[i = l&31][k = l>>5] and B[k = l>>5][j = l&31]; we let lane-half h consume
// k = 4h+s at sub-step s so that one ds_read_b128 per operand covers 4 MFMAs
// (any k permutation is legal as long as A and B agree).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "conv_args.h"
#include "conv_plan.h"
#include "conv_tile.h"

namespace lrp {

// Out-of-image taps / ragged tails read this instead of branching around the load: the
// select is two v_cndmask on the address, the load itself stays unconditional and the
// eight loads of a chunk issue back to back.
__device__ __attribute__((aligned(16))) float lrp_zero_page[4] = {0.f, 0.f, 0.f, 0.f};   // non-const: stays in the GLOBAL address space (a const page makes the select generic -> flat_load, which also counts on lgkmcnt)

// waves per SIMD the register allocator must leave room for: LDS already limits a CU to
// floor(160 KB / LDS per block) blocks of NW waves

// BREG (HALO, bf16x3, N <= 64 layers): the weights never touch LDS.  With K <= 2 x 32 channels per group the whole A
// operand of a group is resident (both LDS buffers hold one 32-channel chunk each), and the B fragments of a
// (tap, chunk) are 4 coalesced 16 B loads per lane from a fragment-major copy of the packed weights (wpk_frag,
// L1/L2 resident: 8 KB per tap), prefetched one tap ahead in registers.  The main loop then has NO barrier per tap —
// only one per channel group — which is what the 12-MFMA-per-tap waves of the N = 64 tiles could not amortise.
// TERMS (split operands): which partial products of (ah + al)(bh + bl) are issued — bit 0: al*bh, bit 1: ah*bl, bit 2: ah*bh
// (al*bl never).  7 = all three: every split launch but the PREC_F16X2 forms below.  PREC_F16X2 only: 5 = bit 1 off, the
// weights' lo half is not read (two MFMAs); bit 4 (23 = 7 | 16, interleaved dual forward) = the same for the odd 32-column
// blocks of the matrix only (Z+: z_tile in the kernel).  Which values exist for which format and epilogue: conv_plan.h conv_epi_exists.
// NS (plain staging only: !HALO, !BREG): LDS stages of the k pipeline.  2 = chunk kc+2 is launched at the barrier of iteration kc
// and must have landed one iteration later — fine when an iteration holds 24-48 MFMAs per wave, but the 64 x 64 tiles of the
// small-grid launches (6 MFMAs per wave and iteration) then run at one L2 / HBM round trip per k-step [MI355X, one image:
// 0.65 us per k-step, 95 us for a K = 4608 launch].  With NS stages NS-1 chunks are in flight and the barrier waits with a
// COUNTED s_waitcnt vmcnt((NS-2) x DMA instructions per chunk) for the oldest only.
// GMASK (EPI_MUL, PREC_FP32 only: the ResNet encoder's gradient walks, resnet_encoder.h explain_grad): `aux` and `join_gate` are
// BYTE masks [images][H][W][N] (1 = the ReLU behind this tensor was active) instead of fp32 gates.  A template axis of its own, so
// that no other instantiation carries its loads (a runtime flag in the shared epilogue costs the VGG walk registers).
// PW (the 128 x 128 weights-in-registers loop only): the launch reads the compact pool interface (ConvArgs::up2_src).  The
// pipelined kernels decide that at run time; in the unrolled chunk of this loop the loader's registers would be carried through the
// dense launch's loop as well, and every reuse of one of them waited for the weight loads in flight [ISA: vmcnt(1) three times a chunk].
// DG (EPI_MUL / EPI_MUL_UP2, PREC_FP32 and PREC_BF16X3, staged and pipelined resident-image tiles): the dual-gate epilogue
// (ConvArgs::aux_b).  An axis of its own for GMASK's reason: the single-gate instantiations compile to what they were.
// C2 (the 128 x 64 weights-in-registers tile, FORM_BREG, dense split-bf16 walk only): the chunk loop of the 8-wave tile instead of this
// tile's first loop (BREG2 below; LRP_CONV_BREG2).  An axis of its own because both loops stay instantiated for the same tile.
template <int WM, int WN, int TM, int TN, int EPI, int PREC, bool HALO = false, bool BREG = false, int TERMS = 7, int NS = 2,
          bool GMASK = false, bool PW = false, bool DG = false, bool C2 = false>
__global__ __launch_bounds__(64 * WM * WN, BREG && WM * WN != 8 && TN == 1 ? 3 : NS > 2 ? 2 : conv_min_waves(WM * WN, TM, TN, HALO)) void conv_igemm_kernel(ConvArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)   // the host pass only needs the launch stub (the buffer-resource builtins are device-only)
  using T = ConvKernelTraits<WM, WN, TM, TN, EPI, PREC, HALO, BREG, TERMS, NS, GMASK, PW, DG, C2>;
  // BREG8: no B stage, so LDS is the two resident images or one 128-row C slab of the epilogue, whichever is larger (128 KB)
  // BREG4: the two resident images + a spare slot per wave (52 KB) or the epilogue's whole 128 x 128 C tile (64 KB; 80 KB pipelined)
  // BREG2: the same 52 KB, three workgroups per CU
  __shared__ __attribute__((aligned(16))) float smem[T::SMEM];

  // ---- XCD-aware block remap: the n_tiles blocks that share an A tile get
  // consecutive logical ids and land on one XCD (one L2) [bijective form].
  const int nblk = a.m_tiles * a.n_tiles;
  int logical;
  {
    const int bid = blockIdx.x, q = nblk >> 3, r = nblk & 7, xcd = bid & 7, idx = bid >> 3;
    logical = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  const int mt = logical / a.n_tiles, nt = logical - mt * a.n_tiles;
  const int m0 = mt * T::BM, n0 = nt * T::BN;
  int pn = 0, py0 = 0, px0 = 0;                        // EPI_IMG_STENCIL: image slot and first OUTPUT pixel of the patch
  if constexpr (EPI == EPI_IMG_STENCIL) {
    const int tpi = a.tiles_x * a.tiles_y;
    pn = mt / tpi;
    const int r = mt - pn * tpi, ty = r / a.tiles_x;
    py0 = ty * IMG_TILE;
    px0 = (r - ty * a.tiles_x) * IMG_TILE;
  }
  int Y0 = 0, x0 = 0, img0 = 0;                          // HALO: first stack row / column of the tile, its image
  if constexpr (HALO) {
    const int mtp = a.tile_map ? a.tile_map[mt] : mt;    // launch order -> tile of the stack (TileOrder)
    const int tyt = mtp / a.cols_t;
    x0 = (mtp - tyt * a.cols_t) * a.tw;
    if (a.tpt > 0) {                                     // per-token tiling (ConvArgs::tpt)
      img0 = tyt / a.tpt;
      Y0 = img0 * a.H + (tyt - img0 * a.tpt) * a.th;
    } else {
      Y0 = tyt * a.th;
      img0 = Y0 / a.H;
    }
  }
  // first stack row that is NOT this tile's any more: the end of the stack, or of the tile's token when tiles are per token
  const int yend = HALO ? (a.tpt > 0 && (img0 + 1) * a.H < a.nyh ? (img0 + 1) * a.H : a.nyh) : 0;
  const float inv_tw = HALO ? 1.0f / (float)a.tw : 0.f, inv_H = HALO ? 1.0f / (float)a.H : 0.f;
  const float inv_H1 = HALO ? 1.0f / (float)(a.H + 1) : 0.f;
  // interleaved dual forward: the scale records of the (at most two, for all but tiny images) images this tile's rows belong
  // to are requested HERE, a main loop ahead of the epilogue that needs them — loaded there, indexed by the row's image,
  // their latency sat on every tile's critical path [MI355X: the forward convs 7 % slower]
  int simg0 = 0;
  float us0 = 1.f, us1 = 1.f, ps0 = 1.f, ps1 = 1.f;
  [[maybe_unused]] const float inv_img_rows = EPI == EPI_FWD_DUAL && a.scale_per_img ? 1.0f / (float)a.img_rows : 0.f;
  if constexpr (EPI == EPI_FWD_DUAL) {
    if (a.dual_il) {
      int simg1 = 0;
      if (a.scale_per_img) {
        simg0 = HALO ? img0 : m0 / a.img_rows;
        simg1 = simg0 + 1 < a.n_imgs ? simg0 + 1 : simg0;
      }
      if constexpr (PREC == PREC_F16X2) { us0 = a.in_unscale[simg0]; us1 = a.in_unscale[simg1]; }
      if (a.pairs_out) { ps0 = a.pairs_scale[simg0]; ps1 = a.pairs_scale[simg1]; }
    }
  }

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave - wm * WN;
  const int HW = a.H * a.W;
  const int K = a.taps * a.CinP;
  const int cpt = a.CinP >> 5;                         // 32-wide k chunks per tap
  const int nk = a.taps * cpt;

  // ---- staging: global -> LDS directly (buffer_load_dwordx4 ... lds), no VGPR round trip.
  // One wave instruction moves 64 x 16 B = 1 KiB = 8 staged rows; the LDS side is linear
  // (M0 base + lane*16), so the XOR swizzle is applied on the per-lane SOURCE offset: lane i of
  // piece q fills row 8q + (i>>3), physical chunk i&7, with logical chunk (i&7) ^ ((row>>1)&7).
  // Wave w issues pieces w*AP .. w*AP+AP-1 of the A tile and w*BP .. of the B tile.
  // Buffer addressing = SGPR base (the descriptor) + SGPR offset (tap / channel chunk: wave-uniform) + one
  // 32-bit VGPR offset per lane that never changes; out-of-image taps, ragged tails and padded channels set the
  // VGPR offset to a value beyond num_records and the hardware writes zeros — no pointer selects, no 64-bit
  // VALU adds, no branches in the loop.  Descriptors are rebased per block, so tensors > 4 GiB are fine.
  int prow = lane >> 3, pchk = lane & 7;             // (not const: the BREG8 loop launders them, see there)
  const int wave_s = __builtin_amdgcn_readfirstlane(wave);
  typedef __attribute__((address_space(3))) void* lptr_t;
  constexpr int OOB = (int)0x80000000;                 // >= any num_records used here
  constexpr int RSRC_FLAGS = 0x00020000;               // raw buffer, DATA_FORMAT_32 (gfx9 V# dword 3)
  const __amdgpu_buffer_rsrc_t rsB =
      __builtin_amdgcn_make_buffer_rsrc((void*)(a.wpk + (size_t)n0 * K), 0, T::BN * K * 4, RSRC_FLAGS);
  int bvo[T::BP];
#pragma unroll
  for (int p = 0; p < T::BP; ++p) {
    const int r = (wave_s * T::BP + p) * 8 + prow;
    bvo[p] = (r * K + ((pchk ^ ((r >> 1) & 7)) << 2)) * 4;
  }
  // A, non-HALO: descriptor base = pixel (m0 - W - 1), so that every tap offset is >= 0
  const float* abase = HALO ? a.in + (size_t)(Y0 > 0 ? Y0 - 1 : 0) * a.W * a.Cin
                       : EPI == EPI_IMG_STENCIL ? a.in + (size_t)pn * HW * a.Cin
                            : a.in + ((long)m0 - (a.taps == 1 ? 0 : a.W + 1)) * (long)a.Cin;
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)abase, 0, 0x7FFFFFFF, RSRC_FLAGS);
  int avo[HALO ? 1 : T::AP];
  unsigned amask[HALO ? 1 : T::AP];
  int acf[HALO ? 1 : T::AP];                              // first channel (within a 32-chunk) of this lane's 16 B
  if constexpr (!HALO) {
    const int rfirst = wave_s * T::AP * 8 + prow;         // tile row of piece p = 0
    const int mfirst = m0 + rfirst;
    int rem = mfirst % HW;
    int h = rem / a.W, w = rem - h * a.W;
#pragma unroll
    for (int p = 0; p < T::AP; ++p) {
      const int r = rfirst + 8 * p, m = m0 + r;
      unsigned mask = 0;
      if constexpr (EPI == EPI_IMG_STENCIL) {
        // patch row r = (py, px) -> pixel (py0 - 1 + py, px0 - 1 + px) of image slot pn; outside the image: zero row
        const int y = py0 - 1 + (r >> 4), x = px0 - 1 + (r & 15);
        const bool ok = y >= 0 && y < a.H && x >= 0 && x < a.W;
        amask[p] = ok ? 1u : 0u;
        const int lc = (pchk ^ ((r >> 1) & 7)) << 2;
        acf[p] = T::SPLIT ? ((lc >> 3) << 3) : lc;
        avo[p] = ok ? ((y * a.W + x) * a.Cin + lc) * 4 : 0;
        continue;
      }
      if (m < a.M) {
        if (a.taps == 1) {
          mask = 1u;
        } else {
          const unsigned row_ok = (h > 0 ? 0x007u : 0u) | 0x038u | (h < a.H - 1 ? 0x1C0u : 0u);   // taps 0-2 / 3-5 / 6-8
          const unsigned col_ok = (w > 0 ? 0x049u : 0u) | 0x092u | (w < a.W - 1 ? 0x124u : 0u);   // taps 0,3,6 / 1,4,7 / 2,5,8
          mask = row_ok & col_ok;
        }
      }
      amask[p] = mask;
      const int lc = (pchk ^ ((r >> 1) & 7)) << 2;
      acf[p] = T::SPLIT ? ((lc >> 3) << 3) : lc;   // 4*chunk (fp32) or 8*(chunk/2) (split8 group)
      avo[p] = (r * a.Cin + lc) * 4;
      if (a.taps != 1) {                                  // next piece: 8 pixels further
        w += 8;
        while (w >= a.W) { w -= a.W; ++h; }
        while (h >= a.H) h -= a.H;
      }
    }
  }

  int tap = 0, cc = 0;                                 // position of the chunk being LOADED
  // HALO: 8-row piece p of the resident image of channel chunk `chunk` -> A buffer `abuf`.
  // piece p = half of resident row hy (wave-uniform): extended stack row E -> image n, row h (h == H: separator)
  const int halo_np = HALO ? a.hrows * (HALO_PITCH / 8) : 0;
  struct HaloPiece { int vo, so; };
  auto prep_halo_piece = [&](int p, int chunk, bool live) {
    const int hy = p >> 1, hx = (p & 1) * 8 + prow;
    const int E = Y0 + img0 - 1 + hy;
    int n, h;
    conv_divmod(E < 0 ? 0 : E, a.H + 1, inv_H1, n, h);
    const int x = x0 - 1 + hx;
    const int lc = (pchk ^ (((hy * a.tw + hx - 1) >> 1) & 7)) << 2;   // halo swizzle, see set_tap
    const int cfirst = T::SPLIT ? ((lc >> 3) << 3) : lc;
    const bool ok = live && E >= 0 && h < a.H && n < a.NB && hx < a.tw + 2 && x >= 0 && x < a.W && (chunk << 5) + cfirst < a.Cin;
    HaloPiece r;
    r.vo = ok ? (x * a.Cin + lc) * 4 : OOB;
    // (n comes out of float math = VALU; the offset is wave-uniform and must reach the instruction in an SGPR)
    const int so = (((E - n) - (Y0 > 0 ? Y0 - 1 : 0)) * a.W * a.Cin + (chunk << 5)) * 4;
    r.so = __builtin_amdgcn_readfirstlane(so < 0 ? 0 : so);
    return r;
  };
  auto fire_halo_piece = [&](const HaloPiece& hp, int p, int abuf) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lptr_t)(smem + abuf * T::STAGE + p * 8 * LDS_STRIDE), 16, hp.vo, hp.so, 0, 0);
  };
  // prep: per-lane offsets of the chunk at (tap, cc) (cheap VALU, placed BEFORE the barrier where it overlaps the
  // MFMAs still in flight); fire: the DMA instructions themselves, right after the barrier.
  struct ChunkPrep { int avo[HALO ? 1 : T::AP]; int aso, bso; };
  auto prep_chunk = [&](bool live) {
    ChunkPrep c;
    const int c0 = cc << 5;
    if constexpr (!HALO) {
#pragma unroll
      for (int p = 0; p < T::AP; ++p) {
        const bool ok = live && ((amask[p] >> tap) & 1u) && (c0 + acf[p] < a.Cin);
        c.avo[p] = ok ? avo[p] : OOB;
      }
    }
    c.aso = ((a.taps == 1 ? 0 : (tap / 3) * a.W + (tap % 3)) * a.Cin + c0) * 4;
    c.bso = live ? (tap * a.CinP + c0) * 4 : 0;
    // taps innermost: the 9 taps of one 32-channel chunk touch the same ~(BM + halo) pixel rows
    // (24 KB), so 8 of 9 re-reads hit L1/L2; tap-major order streamed BM x Cin x 4 B per tap
    // through a 64 KB-per-block share of the XCD's L2 and missed on every tap (FETCH_SIZE 7x).
    if (++tap == a.taps) { tap = 0; ++cc; }
    return c;
  };
  auto fire_chunk = [&](const ChunkPrep& c, int buf) {
    float* As = smem + buf * T::STAGE;
    float* Bs = As + T::ABUF;
    if constexpr (!HALO) {
#pragma unroll
      for (int p = 0; p < T::AP; ++p)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lptr_t)(As + (wave_s * T::AP + p) * 8 * LDS_STRIDE), 16, c.avo[p], c.aso, 0, 0);
    }
#pragma unroll
    for (int p = 0; p < T::BP; ++p)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lptr_t)(Bs + (wave_s * T::BP + p) * 8 * LDS_STRIDE), 16, bvo[p], c.bso, 0, 0);
  };

  // Two-level (blocked) summation: the MFMA is a strictly k-ordered fp32 fma chain, so a
  // K = 4608 reduction in ONE accumulator carries ~sqrt(K) ulp of round-off.  Every FLUSH
  // chunks (256 k) the running block is folded into `tot` and restarted: chains of 256 + K/256.
  // (bf16x3: one MFMA already folds 16 k internally and the chain is K/16 long — no second level.)
  // (the fp16-pair forward, whose three-term product is fp32-grade, is blocked as well: without the second level its
  //  accumulator's 3 x K/16 roundings would be the largest error left)
  f32x16 acc[TM][TN], tot[T::BLOCKED ? TM : 1][T::BLOCKED ? TN : 1];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        acc[i][j][r] = 0.f;
        if constexpr (T::BLOCKED) tot[i][j][r] = 0.f;
      }

  // DMA schedule: chunk kc+2 is launched right AFTER the barrier of iteration kc (the barrier proves every wave
  // has finished reading buffer kc&1) and is waited for at the barrier of iteration kc+1, so a load has a whole
  // iteration (48 MFMAs per wave on the 8-wave tile) to land — launching it at the top of iteration kc+1 instead
  // left it half of that, which the HBM / MALL latency of the A rows did not fit into in the bf16x3 mode.
  // ---- compact pool interface in the PIPELINED halo kernels (!BREG; ConvArgs::up2_pairs): the producer has written
  // S_c = acc x (compact gate) at POOLED resolution as bf16 pairs, and the resident image of the next channel chunk is built
  // from (S_c, position bytes) through registers while the current chunk's taps run, instead of arriving by DMA from the
  // 4x-expanded, 75 %-zero tensor.  Item = (resident row, window column, 8-channel group): it loads its window's pairs
  // (32 B) and position bytes (8 B) and writes the row's two pixels of that window — the value where the position matches,
  // zeros elsewhere (and zeros for separator rows / rows outside the stack).  At most two items per thread and chunk (the
  // launcher checks), handled one after the other so that only ten registers are in flight: item 0 is loaded right after
  // the barrier of tap 3 and written before the barrier of tap 5, item 1 after tap 5 / before tap 7; every write is two
  // barriers ahead of the chunk's first read, into the A buffer last read a chunk ago.  Works on stack tiles and per-token tiles.
  typedef unsigned u32x2w __attribute__((ext_vector_type(2)));
  struct PwItem { u32x4 hi, lo; u32x2w q; };
  // (BREG4: the same items, sequenced by the chunk's steps instead — see its loop)
  [[maybe_unused]] const bool pw = T::BREG4 ? PW : T::BREG2 ? false : HALO && !BREG && PREC == PREC_BF16X3 && a.up2_src != nullptr;
  [[maybe_unused]] int pw_wx0 = 0, pw_nwx = 1, pw_items = 0, pw_ri0 = 0, pw_ri1 = 0;
  [[maybe_unused]] float pw_inv_nwx = 1.f;
  if constexpr (HALO && (!BREG || (PW && T::BREG4)) && PREC == PREC_BF16X3) {
    if (pw) {
      pw_wx0 = (x0 - 1) >> 1;                           // (arithmetic shift: the window column outside the image for x0 = 0)
      pw_nwx = ((x0 + a.tw) >> 1) - pw_wx0 + 1;
      pw_inv_nwx = 1.0f / (float)pw_nwx;
      pw_items = a.hrows * pw_nwx * 4;
      pw_ri0 = a.row2img ? a.row2img[img0 < a.NB ? img0 : a.NB - 1] : img0;
      pw_ri1 = a.row2img ? a.row2img[img0 + 1 < a.NB ? img0 + 1 : a.NB - 1] : img0 + 1;
    }
  }
  struct PwPos { const float* sp; const unsigned char* qp; bool valid; int hy, wx, g, dy; };
  [[maybe_unused]] auto pw_locate = [&](int it, int chunk) {
    PwPos r;
    r.g = it & 3;
    int wxi;
    conv_divmod(it >> 2, pw_nwx, pw_inv_nwx, r.hy, wxi);
    r.wx = pw_wx0 + wxi;
    const int Hp = a.H >> 1, Wp = a.W >> 1;
    const int E = Y0 + img0 - 1 + r.hy;
    int n, h;
    conv_divmod(E < 0 ? 0 : E, a.H + 1, inv_H1, n, h);
    r.valid = it < pw_items && E >= 0 && h < a.H && n < a.NB && r.wx >= 0 && r.wx < Wp && (chunk << 5) + r.g * 8 < a.Cin;
    r.dy = h & 1;
    // unconditional loads from a clamped (always valid) place; an invalid item's values are zeroed at the store
    const int nc = r.valid ? n : 0, wyc = r.valid ? (h >> 1) : 0, wxc = r.valid ? r.wx : 0, co = r.valid ? (chunk << 5) + r.g * 8 : 0;
    const int rel = nc - img0;
    // (PW: a resident image spans two images at most — conv_plan takes the form for hrows <= H only — and a look-up here would drain
    //  the weight loads in flight; an item that is not valid loads from a clamped place of image pw_ri0)
    const int img = PW ? (rel == 1 ? pw_ri1 : pw_ri0) : rel == 0 ? pw_ri0 : rel == 1 ? pw_ri1 : (a.row2img ? a.row2img[nc] : nc);
    r.sp = a.up2_src + (((size_t)nc * Hp + wyc) * Wp + wxc) * a.Cin + co;
    r.qp = a.up2_gpos + (((size_t)img * Hp + wyc) * Wp + wxc) * a.Cin + co;
    return r;
  };
  [[maybe_unused]] auto pw_load = [&](PwItem& w, int it, int chunk) {
    const PwPos r = pw_locate(it, chunk);
    w.hi = *reinterpret_cast<const u32x4*>(r.sp);
    w.lo = *reinterpret_cast<const u32x4*>(r.sp + 4);
    w.q = *reinterpret_cast<const u32x2w*>(r.qp);
  };
  [[maybe_unused]] auto pw_store = [&](const PwItem& w, int it, int chunk, int abuf) {
    if (it >= pw_items) return;
    const PwPos r = pw_locate(it, chunk);
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const int hx = 2 * r.wx + dx - (x0 - 1);
      if (hx < 0 || hx >= HALO_PITCH) continue;
      const unsigned j = (unsigned)((r.dy << 1) | dx);  // this pixel's position in its window
      u32x4 mh, ml;
#pragma unroll
      for (int d = 0; d < 4; ++d) {                       // 16-bit lane c keeps its value iff channel c's arg-max sits at position j
        const unsigned p0 = (w.q[d >> 1] >> (16 * (d & 1))) & 0xFFu, p1 = (w.q[d >> 1] >> (16 * (d & 1) + 8)) & 0xFFu;
        const unsigned m = r.valid ? ((p0 == j ? 0x0000FFFFu : 0u) | (p1 == j ? 0xFFFF0000u : 0u)) : 0u;
        mh[d] = w.hi[d] & m;
        ml[d] = w.lo[d] & m;
      }
      const int row = r.hy * HALO_PITCH + hx;
      const int swzu = ((r.hy * a.tw + hx - 1) >> 1) & 7;
      const int dst = abuf * T::STAGE + row * LDS_STRIDE + (((2 * r.g) ^ swzu) << 2);
      *reinterpret_cast<u32x4*>(smem + dst) = mh;
      *reinterpret_cast<u32x4*>(smem + (dst ^ 4)) = ml;
    }
  };
  [[maybe_unused]] PwItem pwi{};
  // compact pool interface into the 128 x 64 weights-in-registers tile (pairs of S_c; per-token tiles, at most 64 channels: conv_plan
  // checks): the whole A operand — both chunks, both LDS buffers — is built up front.
  [[maybe_unused]] auto breg_window_loader = [&]() {
    // compact pool interface (pairs of S_c, per-token tiles: the launcher checks): item = (window of the resident image,
    // 8-channel group)
    const int Hp = a.H >> 1, Wp = a.W >> 1;
    const int h0 = Y0 - img0 * a.H;                      // the tile's first image row (tiles are per token)
    const int wy0 = (h0 - 1) >> 1, wx0 = (x0 - 1) >> 1;  // (arithmetic shifts: -1 >> 1 = -1, the window row / column outside the image)
    const int nwx = ((x0 + a.tw) >> 1) - wx0 + 1, nwy = ((h0 + a.th) >> 1) - wy0 + 1;
    const int items = nwy * nwx * 8;
    const int ntok = img0 < a.NB ? img0 : a.NB - 1;
    const int img = a.row2img ? a.row2img[ntok] : ntok;
    const float inv_nwx = 1.0f / (float)nwx;
    constexpr int UW = 2;                                // items in flight per thread (2 x 16 B + 8 B of loads each)
    typedef unsigned u32x2_ __attribute__((ext_vector_type(2)));
    for (int it0 = tid; it0 < items; it0 += T::NT * UW) {
      f32x4 pv[UW][2];
      u32x2_ qv[UW];
      int wyv[UW], wxv[UW], cgv[UW];
      bool okv[UW];
#pragma unroll
      for (int u = 0; u < UW; ++u) {
        const int item = it0 + u * T::NT;
        const int cg = item & 7, wdx = item >> 3;
        int wr, wc;
        conv_divmod(wdx, nwx, inv_nwx, wr, wc);
        const int wy = wy0 + wr, wx = wx0 + wc;
        cgv[u] = cg; wyv[u] = wy; wxv[u] = wx;
        okv[u] = item < items && wy >= 0 && wy < Hp && wx >= 0 && wx < Wp && cg * 8 < a.Cin;
        // unconditional loads from a clamped (always valid) window; the values of an invalid item are zeroed below
        const int wyc = wy < 0 ? 0 : (wy >= Hp ? Hp - 1 : wy), wxc = wx < 0 ? 0 : (wx >= Wp ? Wp - 1 : wx);
        const int cgc = cg * 8 < a.Cin ? cg : 0;
        const size_t wo = ((size_t)wyc * Wp + wxc) * a.Cin + cgc * 8;
        const float* pp = a.up2_src + (size_t)ntok * Hp * Wp * a.Cin + wo;
        pv[u][0] = *reinterpret_cast<const f32x4*>(pp); pv[u][1] = *reinterpret_cast<const f32x4*>(pp + 4);
        qv[u] = *reinterpret_cast<const u32x2_*>(a.up2_gpos + (size_t)img * Hp * Wp * a.Cin + wo);
      }
#pragma unroll
      for (int u = 0; u < UW; ++u) {
        if (it0 + u * T::NT >= items) continue;
        const u32x4 z4u = {0u, 0u, 0u, 0u};
        const u32x4 hiw = okv[u] ? __builtin_bit_cast(u32x4, pv[u][0]) : z4u;   // S_c as [hi8 | lo8]
        const u32x4 low = okv[u] ? __builtin_bit_cast(u32x4, pv[u][1]) : z4u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {                    // the window's four pixels: position j = 2 dy + dx
          const int hy = 2 * wyv[u] + (j >> 1) - (h0 - 1), hx = 2 * wxv[u] + (j & 1) - (x0 - 1);
          if (hy < 0 || hy >= a.hrows || hx < 0 || hx >= HALO_PITCH) continue;
          // 16-bit lane c of a dword pair keeps its value iff channel c's arg-max sits at position j
          u32x4 mh, ml;
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            const unsigned p0 = (qv[u][d >> 1] >> (16 * (d & 1))) & 0xFFu, p1 = (qv[u][d >> 1] >> (16 * (d & 1) + 8)) & 0xFFu;
            const unsigned m = (p0 == (unsigned)j ? 0x0000FFFFu : 0u) | (p1 == (unsigned)j ? 0xFFFF0000u : 0u);
            mh[d] = hiw[d] & m;
            ml[d] = low[d] & m;
          }
          const int row = hy * HALO_PITCH + hx;
          const int swzu = ((hy * a.tw + hx - 1) >> 1) & 7;
          const int dst = (cgv[u] >> 2) * T::STAGE + row * LDS_STRIDE + (((2 * (cgv[u] & 3)) ^ swzu) << 2);
          *reinterpret_cast<u32x4*>(smem + dst) = mh;
          *reinterpret_cast<u32x4*>(smem + (dst ^ 4)) = ml;
        }
      }
    }
  };
  // the chunk loop's prologue: chunk 0 of the resident image; chunk 1 follows in the loop.  (BREG2 with PW — the folded launch,
  // at most two chunks: both, through the window loader above.  Chunk 1 by pw_load / pw_store items during chunk 0's steps, as on
  // the BREG4 loop, was measured and lost to the first loop by 2 %; this form wins 7 %: profiles/breg2_ab.txt.)
  [[maybe_unused]] auto bregc_chunk0 = [&]() {
    if constexpr (PW && T::BREG2) {
      breg_window_loader();
    } else if constexpr (PW) {
      pw_load(pwi, tid, 0); pw_store(pwi, tid, 0, 0);
      if (tid + T::NT < pw_items) { pw_load(pwi, tid + T::NT, 0); pw_store(pwi, tid + T::NT, 0, 0); }
    } else
    for (int p = wave_s; p < halo_np; p += T::NW) fire_halo_piece(prep_halo_piece(p, 0, true), p, 0);
  };
  if constexpr (T::BREG2) {
    // (its prologue runs behind the first weight loads, in front of the loop: see there)
  } else if constexpr (T::BREGC) {
    bregc_chunk0();
  } else if constexpr (BREG) {
    if (PREC == PREC_BF16X3 && a.up2_src) {
      breg_window_loader();
    } else
    for (int p = wave_s; p < halo_np; p += T::NW) {         // channel chunks 0 and 1 -> LDS buffers 0 and 1
      fire_halo_piece(prep_halo_piece(p, 0, true), p, 0);
      fire_halo_piece(prep_halo_piece(p, 1, cpt > 1), p, 1);
    }
  } else {
    if constexpr (HALO) {
      if (pw) {
        pw_load(pwi, tid, 0); pw_store(pwi, tid, 0, 0);
        if (tid + T::NT < pw_items) { pw_load(pwi, tid + T::NT, 0); pw_store(pwi, tid + T::NT, 0, 0); }
      } else {
        for (int p = wave_s; p < halo_np; p += T::NW) fire_halo_piece(prep_halo_piece(p, 0, true), p, 0);
        if (wave_s < halo_np) fire_halo_piece(prep_halo_piece(wave_s, 1, cpt > 1), wave_s, 1);   // slot 0 of chunk 1 (see the loop)
      }
    }
    fire_chunk(prep_chunk(true), 0);
    fire_chunk(prep_chunk(nk > 1), 1);
#pragma unroll
    for (int s_ = 2; s_ < NS; ++s_) fire_chunk(prep_chunk(nk > s_), s_);
  }
  if constexpr (!T::BREG2) conv_dma_oldest_landed_barrier<T>();

  const int a_off = HALO ? 0 : (wm * TM * 32 + (lane & 31)) * LDS_STRIDE;
  const int b_off = T::ABUF + (wn * TN * 32 + (lane & 31)) * LDS_STRIDE;
  // HALO: per A fragment row, the LDS row of its pixel in the resident image (padding rows of the tile read
  // pixel (1,1): their C rows are never stored), and per tap the float offset of its first 16 B chunk
  int fbase[HALO ? TM : 1], fu[HALO ? TM : 1], faddr[HALO ? TM : 1];
  const int hh_ = lane >> 5;
  if constexpr (HALO) {
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int r = (wm * TM + i) * 32 + (lane & 31);
      int ty, tx, n_, h_;
      conv_divmod(r, a.tw, inv_tw, ty, tx);
      const int Y = Y0 + ty;
      conv_divmod(Y, a.H, inv_H, n_, h_);
      const bool ok = r < a.th * a.tw && Y < yend && x0 + tx < a.W;
      const int hy = ok ? ty + 1 + n_ - img0 : 1, hx = ok ? tx + 1 : 1;
      fbase[i] = hy * HALO_PITCH + hx;
      fu[i] = hy * a.tw + hx - 1;
    }
  }
  auto tap_shift = [&](int t) { return (t / 3 - 1) * HALO_PITCH + (t % 3 - 1); };
  // first chunk of lane-half hh at step 0 is 2hh (bf16x3: hi of split8 group hh) / hh (fp32); the others are XORs of it
  // Halo swizzle: the 16 B chunk index is XORed with (u >> 1) & 7, u = hy*tw + hx - 1 = the pixel's index in the
  // DENSE tile (the LDS rows have pitch 16 but only tw = 14 of them per image row are tile pixels).  The 32 lanes
  // of a fragment read 32 consecutive tile pixels, i.e. consecutive u (shifted as a whole by the tap), and 16
  // consecutive u give 16 distinct (row parity, chunk ^ swizzle) bank slots; the LDS-row based swizzle of the
  // non-halo layout would collide on the two rows behind every wrap of tx.
  auto set_tap = [&](int t) {
    const int tsh = tap_shift(t), ush = (t / 3 - 1) * a.tw + (t % 3 - 1);
#pragma unroll
    for (int i = 0; i < (HALO ? TM : 0); ++i) {
      const int row = fbase[i] + tsh, u = fu[i] + ush;
      faddr[i] = row * LDS_STRIDE + ((((T::SPLIT ? 2 : 1) * hh_) ^ ((u >> 1) & 7)) << 2);
    }
  };
  // Fragment registers are double-buffered one step ahead, and the first fragments of the NEXT
  // chunk are fetched right after the barrier: the last MFMA group of the current chunk runs on
  // registers while those reads are in flight.  (All reads of `buf` are issued AND completed
  // before the barrier => the DMA of the following iteration cannot race them.)
  // fp32 : 4 steps of 8 k per chunk; lane-half h consumes k = 4h+s -> logical chunk 2kk+h.
  // bf16x3: 2 steps of 16 k; lane-half h consumes k = 8h+j -> split8 group 2s+h = chunks 4s+2h (hi), 4s+2h+1 (lo).
  const int swz = (lane >> 1) & 7, hh = lane >> 5;
  int koff[4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
    koff[q] = T::SPLIT ? (((4 * (q >> 1) + 2 * hh + (q & 1)) ^ swz) << 2)     // q = 2*step + {hi,lo}
                                  : (((2 * q + hh) ^ swz) << 2);
  // TERMS bit 4: is column tile j of this wave an ODD 32-column block of the matrix (interleaved rows: Z+)?  By the block's place
  // in the MATRIX, not in the wave: with one column tile per wave (the 64 x 64, 128 x 64 and 128 x 32 tiles) the wave's own index
  // is always 0, and those tiles computed Z+ with all three terms — the denominators, and with them an image's heat-map in the
  // fp16-pair walk, depended on which tile the batch size picked.  Two column tiles per wave: j & 1, known at compile time.
  const int ztile0 = TN % 2 == 0 ? 0 : ((n0 >> 5) + (wave_s % WN) * TN) & 1;
  auto z_tile = [&](int j) { return ((ztile0 + j) & 1) != 0; };
  struct Frag { u32x4 a[T::SPLIT ? 2 * TM : TM], b[T::SPLIT ? 2 * TN : TN]; };
  // HALO: A addresses come from faddr[] (set_tap); chunk c ^ swizzle = (c0 ^ swizzle) ^ (c - c0) for disjoint bits
  auto read_frag = [&](Frag& f, const float* Ab, const float* Bb, int st) {
    if constexpr (HALO) {
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        if constexpr (T::SPLIT) {
          f.a[2 * i] = *reinterpret_cast<const u32x4*>(Ab + (faddr[i] ^ ((4 * st) << 2)));
          f.a[2 * i + 1] = *reinterpret_cast<const u32x4*>(Ab + (faddr[i] ^ ((4 * st + 1) << 2)));
        } else {
          f.a[i] = *reinterpret_cast<const u32x4*>(Ab + (faddr[i] ^ ((2 * st) << 2)));
        }
      }
    } else if constexpr (T::SPLIT) {
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        f.a[2 * i] = *reinterpret_cast<const u32x4*>(Ab + i * 32 * LDS_STRIDE + koff[2 * st]);
        f.a[2 * i + 1] = *reinterpret_cast<const u32x4*>(Ab + i * 32 * LDS_STRIDE + koff[2 * st + 1]);
      }
    } else {
#pragma unroll
      for (int i = 0; i < TM; ++i) f.a[i] = *reinterpret_cast<const u32x4*>(Ab + i * 32 * LDS_STRIDE + koff[st]);
    }
    if constexpr (T::SPLIT) {
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        f.b[2 * j] = *reinterpret_cast<const u32x4*>(Bb + j * 32 * LDS_STRIDE + koff[2 * st]);
        if (PREC != PREC_F16X2 || ((TERMS & 2) != 0 && !((TERMS & 16) != 0 && TN % 2 == 0 && (j & 1))))   // (two-term form: the lo chunk is never read)
          f.b[2 * j + 1] = *reinterpret_cast<const u32x4*>(Bb + j * 32 * LDS_STRIDE + koff[2 * st + 1]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < TN; ++j) f.b[j] = *reinterpret_cast<const u32x4*>(Bb + j * 32 * LDS_STRIDE + koff[st]);
    }
  };
  auto mfma_frag = [&](const Frag& f) {
    if constexpr (PREC == PREC_F16X2) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const f16x8 ah = __builtin_bit_cast(f16x8, f.a[2 * i]), al = __builtin_bit_cast(f16x8, f.a[2 * i + 1]);
          const f16x8 bh = __builtin_bit_cast(f16x8, f.b[2 * j]);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc[i][j], 0, 0, 0);    // small terms first
          // TERMS 7: the weights' lo half too.  TERMS bit 4 (interleaved dual forward): not for the odd column tiles = Z+
          if ((TERMS & 2) != 0 && !((TERMS & 16) != 0 && z_tile(j)))        // (TN even: folds once the j loop is unrolled; else wave-uniform)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, __builtin_bit_cast(f16x8, f.b[2 * j + 1]), acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc[i][j], 0, 0, 0);
        }
    } else if constexpr (PREC == PREC_BF16X3) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const bf16x8 ah = __builtin_bit_cast(bf16x8, f.a[2 * i]), al = __builtin_bit_cast(bf16x8, f.a[2 * i + 1]);
          const bf16x8 bh = __builtin_bit_cast(bf16x8, f.b[2 * j]), bl = __builtin_bit_cast(bf16x8, f.b[2 * j + 1]);
          if constexpr ((TERMS & 1) != 0) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[i][j], 0, 0, 0);    // small terms first
          if constexpr ((TERMS & 2) != 0) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc[i][j], 0, 0, 0);
          if constexpr ((TERMS & 4) != 0) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[i][j], 0, 0, 0);
        }
    } else {
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(__builtin_bit_cast(f32x4, f.a[i])[s],
                                                             __builtin_bit_cast(f32x4, f.b[j])[s], acc[i][j], 0, 0, 0);
    }
  };

  if constexpr (T::BREGC) {
    // ---- 8-wave tile (and, BREG4, the 4-wave 128 x 128 tile), weights in registers.  The pipelined form of this tile ends every tap in vmcnt(0) + a workgroup
    // barrier (the weight stage it vacates is refilled for tap + 2), which keeps all eight waves — both waves of every SIMD —
    // in the same phase.  Here B never touches LDS: a wave takes its 64 columns' fragments of one k16 step with four coalesced
    // 16 B loads from the fragment-major copy (wpk_frag: [kc][step][hi|lo][lane half][N] x 16 B, the BREG layout over all N
    // columns), two steps ahead of their use in a ring of three register sets, and waits for them with a counted vmcnt.
    // The A fragments of step s + 1 are re-read row block by row block behind the six MFMAs that consumed that block at
    // step s (one register set: 128 accumulators + 48 B + 32 A).  The only workgroup barrier is the one where the A buffers
    // change hands, once per channel chunk: the next chunk's resident image arrives by six DMA pieces per wave spread over
    // the chunk's steps and is waited for (in-order vmcnt) in front of that barrier.  A chunk's 18 steps are unrolled into
    // ONE basic block — dead pieces and prefetches past the end are clamped or go to a spare LDS slot instead of being
    // branched around — so that hipcc counts every wait.  Same MFMA chain per output element as every other form: chunk-major,
    // taps innermost, two k16 steps, al*bh, ah*bl, ah*bh.
    // BREG2 (TM x TN = 2 x 1, the N <= 64 launches): the same 24 pieces; a weight step is two loads and six MFMAs.  PW there is the
    // folded launch (per-token tiles, at most two chunks): the window loader has built both chunks in the prologue, no piece arrives
    // during the loop.  The first two weight steps are requested in front of the resident image (see below).
    // BREG4 (TM x TN = 2 x 2): a 12-row resident image is 24 pieces = six per wave as well, and two outstanding weight steps
    // are again 2 x 2 TN = 8 loads.  The fp16-pair dual forward rides on the same loop: TERMS 23 leaves out the lo half of the
    // odd column tiles (Z+; three loads per step, six outstanding), and the blocked accumulation folds acc into tot behind the
    // same taps as the pipelined loop — kc = 9 chunk + tap, (kc & 7) == 7 <=> ((chunk + tap) & 7) == 7 — under a wave-uniform
    // branch that holds VALU work only, so the weight waits stay counted.
    // does column tile j read the weights' lo half (mfma_frag's rule)
    auto uses_lo = [](int j) { return PREC != PREC_F16X2 || ((TERMS & 2) != 0 && !((TERMS & 16) != 0 && (j & 1))); };
    constexpr int LPS = PREC == PREC_F16X2 && (TERMS & 16) != 0 ? 2 * TN - TN / 2 : 2 * TN;   // weight loads per k16 step
    const int NF = a.n_tiles * T::BN;                       // columns of the fragment-major copy (N % BN == 0)
    const int nsteps = 2 * nk;
    const __amdgpu_buffer_rsrc_t rsF = __builtin_amdgcn_make_buffer_rsrc((void*)a.wpk_frag, 0, nsteps * 4 * NF * 16, RSRC_FLAGS);
    const int fvo = ((lane >> 5) * NF + n0 + wn * TN * 32 + (lane & 31)) * 16;
    u32x4 bq[3][2 * TN];                                 // ring of three k16 steps: [hi|lo] x TN
    u32x4 aq[2 * TM];                                    // the step being consumed: [row block][hi|lo]
    auto load_b = [&](u32x4* b, int gs) {                // gs = (chunk * 9 + tap) * 2 + step
      const int so = (gs < nsteps ? gs : nsteps - 1) * 4 * NF * 16;
#pragma unroll
      for (int hl = 0; hl < 2; ++hl)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          if (hl == 0 || uses_lo(j))
            b[hl * TN + j] = __builtin_amdgcn_raw_buffer_load_b128(rsF, fvo + j * 32 * 16, so + hl * 2 * NF * 16, 0);
    };
    load_b(bq[0], 0);
    load_b(bq[1], 1);
    if constexpr (T::BREG2) {
      // the first two weight steps depend on nothing the image barrier protects: requested in front of the resident image, their
      // round trip runs under the image's (a tile of the N <= 64 launches is 18 or 36 steps long: every exposed round trip counts)
      bregc_chunk0();
      conv_dma_landed_barrier();
    }
    set_tap(0);
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      aq[2 * i] = *reinterpret_cast<const u32x4*>(smem + faddr[i]);
      aq[2 * i + 1] = *reinterpret_cast<const u32x4*>(smem + (faddr[i] ^ 4));
    }
    for (int c = 0; c < cpt; ++c) {
      const int cb = c & 1;
      const float* Ab = smem + cb * T::STAGE;
      const float* An = smem + (cb ^ 1) * T::STAGE;
      // the per-tap fragment addresses and most of a piece's offsets do not depend on the chunk: left alone, hipcc hoists all of
      // them (nine taps x four row blocks, six pieces) out of the chunk loop and spills them.  They are a few VALU ops each.
#pragma unroll
      for (int i = 0; i < TM; ++i) asm volatile("" : "+v"(fbase[i]), "+v"(fu[i]));
      asm volatile("" : "+v"(prow), "+v"(pchk));
#pragma unroll
      for (int s = 0; s < 18; ++s) {
        load_b(bq[(s + 2) % 3], c * 18 + s + 2);
        if constexpr (PW && T::BREG2) {
          // (both chunks were built in the prologue: nothing arrives during the loop)
        } else if constexpr (PW) {
          // compact pool interface: behind the hand-over barrier of chunk c - 1 the other buffer is free for all of chunk c.  The two
          // items of a thread go through the same ten registers one after the other: loaded early, written mid-chunk; the
          // lgkmcnt(0) in front of the next hand-over covers the writes.  (Unconditional: a dead item loads from a clamped
          // address and writes nothing or zeros, a chunk past the end zeros — like the dead pieces below.)
          if (s == 0) pw_load(pwi, tid, c + 1);
          if (s == 6) { pw_store(pwi, tid, c + 1, cb ^ 1); pw_load(pwi, tid + T::NT, c + 1); }
          if (s == 12) pw_store(pwi, tid + T::NT, c + 1, cb ^ 1);
        } else if (s % 3 == 0) {                         // piece slot s / 3 of chunk c + 1 -> the buffer chunk c - 1 was read from
          const int p = (s / 3) * T::NW + wave_s;
          const bool livep = p < halo_np;
          const HaloPiece hp = prep_halo_piece(p, c + 1, livep && c + 1 < cpt);
          const int dst = livep ? (cb ^ 1) * T::STAGE + p * 8 * LDS_STRIDE : 2 * T::STAGE + wave_s * 8 * LDS_STRIDE;   // (dead piece: zeros into the spare slot)
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lptr_t)(smem + dst), 16, hp.vo, hp.so, 0, 0);
        }
        if (s == 17) {
          // A hand-over.  Loads complete in order: all but the two youngest weight steps done = every piece of chunk c + 1
          // this wave fired (the last one at step 15) has landed; lgkmcnt(0) = this wave's reads of chunk c are done, so
          // behind the barrier its buffer may be refilled.  (Not __syncthreads(): its fence would drain the weight loads.)
          asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(2 * LPS) : "memory");
        }
        const int nst = (s + 1) & 1;
        if (nst == 0) set_tap(((s + 1) >> 1) % 9);
        const float* Ax = s == 17 ? An : Ab;
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          if constexpr (PREC == PREC_F16X2) {
            const f16x8 ah = __builtin_bit_cast(f16x8, aq[2 * i]), al = __builtin_bit_cast(f16x8, aq[2 * i + 1]);
#pragma unroll
            for (int j = 0; j < TN; ++j) {
              const f16x8 bh = __builtin_bit_cast(f16x8, bq[s % 3][j]);
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc[i][j], 0, 0, 0);
              if (uses_lo(j)) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, __builtin_bit_cast(f16x8, bq[s % 3][TN + j]), acc[i][j], 0, 0, 0);
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc[i][j], 0, 0, 0);
            }
          } else {
            const bf16x8 ah = __builtin_bit_cast(bf16x8, aq[2 * i]), al = __builtin_bit_cast(bf16x8, aq[2 * i + 1]);
#pragma unroll
            for (int j = 0; j < TN; ++j) {
              const bf16x8 bh = __builtin_bit_cast(bf16x8, bq[s % 3][j]), bl = __builtin_bit_cast(bf16x8, bq[s % 3][TN + j]);
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[i][j], 0, 0, 0);
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc[i][j], 0, 0, 0);
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[i][j], 0, 0, 0);
            }
          }
          // this row block's fragments of the next step, behind the MFMAs that have just read the old ones
          aq[2 * i] = *reinterpret_cast<const u32x4*>(Ax + (faddr[i] ^ ((4 * nst) << 2)));
          aq[2 * i + 1] = *reinterpret_cast<const u32x4*>(Ax + (faddr[i] ^ ((4 * nst + 1) << 2)));
          __builtin_amdgcn_sched_barrier(0);             // (pinned: hoisted above the MFMAs the reads would need a second register set)
        }
        if constexpr (T::BLOCKED) {
          if ((s & 1) && ((c + (s >> 1)) & (T::FLUSH - 1)) == T::FLUSH - 1) {   // behind tap s >> 1: where the pipelined loop flushes
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
              for (int j = 0; j < TN; ++j) {
                tot[i][j] += acc[i][j];
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
              }
          }
        }
      }
    }
  } else if constexpr (BREG) {
    // B fragments of (kc = chunk*9 + tap): [step][hi|lo] x TN, one 16 B load each
    const __amdgpu_buffer_rsrc_t rsF = __builtin_amdgcn_make_buffer_rsrc((void*)a.wpk_frag, 0, nk * 8 * T::BN * 16, RSRC_FLAGS);
    const int fvo = ((lane >> 5) * T::BN + wn * TN * 32 + (lane & 31)) * 16;
    struct BFrag { u32x4 v[4 * TN]; };
    auto load_b = [&](BFrag& b, int kc) {
#pragma unroll
      for (int q = 0; q < 4; q += ((PREC == PREC_F16X2 && !(TERMS & 2)) ? 2 : 1))    // q = 2*step + (0 hi | 1 lo); two-term fp16: hi only
#pragma unroll
        for (int j = 0; j < TN; ++j)
          b.v[q * TN + j] = __builtin_amdgcn_raw_buffer_load_b128(rsF, fvo + j * 32 * 16, ((kc * 4 + q) * 2) * T::BN * 16, 0);
    };
    struct AFrag { u32x4 v[4 * TM]; };                   // [step][hi|lo] x TM
    auto load_a = [&](AFrag& f, const float* Ab) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int i = 0; i < TM; ++i)
          f.v[q * TM + i] = *reinterpret_cast<const u32x4*>(Ab + (faddr[i] ^ (((q >> 1) * 4 + (q & 1)) << 2)));
    };
    auto mma = [&](const AFrag& f, const BFrag& b) {
#pragma unroll
      for (int st = 0; st < 2; ++st)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            if constexpr (PREC == PREC_F16X2) {
              const f16x8 ah = __builtin_bit_cast(f16x8, f.v[(2 * st) * TM + i]), al = __builtin_bit_cast(f16x8, f.v[(2 * st + 1) * TM + i]);
              const f16x8 bh = __builtin_bit_cast(f16x8, b.v[(2 * st) * TN + j]);
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc[i][j], 0, 0, 0);
              if constexpr ((TERMS & 2) != 0)
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, __builtin_bit_cast(f16x8, b.v[(2 * st + 1) * TN + j]), acc[i][j], 0, 0, 0);
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc[i][j], 0, 0, 0);
            } else {
              const bf16x8 ah = __builtin_bit_cast(bf16x8, f.v[(2 * st) * TM + i]), al = __builtin_bit_cast(bf16x8, f.v[(2 * st + 1) * TM + i]);
              const bf16x8 bh = __builtin_bit_cast(bf16x8, b.v[(2 * st) * TN + j]), bl = __builtin_bit_cast(bf16x8, b.v[(2 * st + 1) * TN + j]);
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[i][j], 0, 0, 0);
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc[i][j], 0, 0, 0);
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[i][j], 0, 0, 0);
            }
          }
    };
    BFrag b0, b1;
    AFrag a0, a1;
    load_b(b0, 0);
    for (int g = 0; g < cpt; g += 2) {                   // groups of two channel chunks = the two LDS buffers
      if (g > 0) {
        __syncthreads();                                 // everyone is done with the previous group's image
        for (int p = wave_s; p < halo_np; p += T::NW) {
          fire_halo_piece(prep_halo_piece(p, g, true), p, 0);
          fire_halo_piece(prep_halo_piece(p, g + 1, g + 1 < cpt), p, 1);
        }
        conv_dma_landed_barrier();
      }
      const int ng = (g + 2 <= cpt ? 2 : 1) * 9;         // (tap, chunk) pairs of this group
      set_tap(0);
      load_a(a0, smem);
      // Two pairs per trip (the register double buffers alternate).  The body is branch-free on purpose — prefetches
      // past the end are clamped re-loads — so that it stays ONE basic block and hipcc can wait for exactly the four
      // older weight loads (vmcnt(4)); with branches around the loads it fell back to vmcnt(0) on every tap.
      int nt = 0, nc = 0;                                // (tap, chunk in group) of the pair being prefetched
      for (int q = 0; q < ng; q += 2) {
        const int kc = g * 9 + q;
        if (++nt == 9) { nt = 0; ++nc; }
        load_b(b1, kc + 1 < nk ? kc + 1 : nk - 1);
        set_tap(nt);
        load_a(a1, smem + (nc > 1 ? 1 : nc) * T::STAGE);
        __builtin_amdgcn_sched_barrier(0);               // keep the prefetches ABOVE the 12 MFMAs they hide behind
        mma(a0, b0);
        __builtin_amdgcn_sched_barrier(0);
        if (++nt == 9) { nt = 0; ++nc; }
        load_b(b0, kc + 2 < nk ? kc + 2 : nk - 1);
        set_tap(nt);
        load_a(a0, smem + (nc > 1 ? 1 : nc) * T::STAGE);
        __builtin_amdgcn_sched_barrier(0);
        if (q + 1 < ng) mma(a1, b1);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  Frag f0, f1;
  int ctap = 0, ccc = 0;                               // HALO: (tap, channel chunk) being COMPUTED; kc = ccc*9 + ctap
  if constexpr (!BREG) {
  set_tap(0);
  read_frag(f0, smem + a_off, smem + b_off, 0);
  }
  int buf = 0;                                         // = kc % NS
  for (int kc = 0; kc < (BREG ? 0 : nk); ++kc) {
    const bool more = (kc + 1) < nk;
    const int nbuf = buf + 1 == NS ? 0 : buf + 1;      // stage of chunk kc + 1
    const int abuf = HALO ? (ccc & 1) : buf;
    const float* Ab = smem + abuf * T::STAGE + a_off;
    const float* Bb = smem + buf * T::STAGE + b_off;
    if constexpr (T::NSTEP == 4) {
      read_frag(f1, Ab, Bb, 1);
      mfma_frag(f0);                                   // step 0
      read_frag(f0, Ab, Bb, 2);
      mfma_frag(f1);                                   // step 1
      read_frag(f1, Ab, Bb, 3);
      mfma_frag(f0);                                   // step 2
    } else {
      read_frag(f1, Ab, Bb, 1);
      mfma_frag(f0);                                   // step 0
    }
    // offsets of chunk kc+2 (-> `buf`) and, HALO, of this tap slot's piece of the next channel chunk's resident
    // image (slot = one piece per wave; that A buffer was last read in the chunk before this one)
    const ChunkPrep cp = prep_chunk(kc + NS < nk);
    HaloPiece hp{};
    int hpp = 0;
    if constexpr (HALO) {
      if (++ctap == 9) { ctap = 0; ++ccc; }
      if (pw) {
        hpp = -1;
        if (ccc + 1 < cpt) {
          if (ctap == 5) pw_store(pwi, tid, ccc + 1, (ccc & 1) ^ 1);
          else if (ctap == 7) pw_store(pwi, tid + T::NT, ccc + 1, (ccc & 1) ^ 1);
        }
      } else {
        hpp = ctap * T::NW + wave_s;
        if (hpp >= halo_np) hpp = -1;
        hp = prep_halo_piece(hpp < 0 ? 0 : hpp, ccc + 1, more && ccc + 1 < cpt);
      }
    }
    conv_dma_oldest_landed_barrier<T>();                       // reads of `buf` done everywhere; DMA of chunk kc+1 landed
    fire_chunk(cp, buf);
    if constexpr (HALO) {
      if (pw) {
        if (ccc + 1 < cpt) {
          if (ctap == 3) pw_load(pwi, tid, ccc + 1);
          else if (ctap == 5 && tid + T::NT < pw_items) pw_load(pwi, tid + T::NT, ccc + 1);
        }
      } else if (hpp >= 0 && more && ccc + 1 < cpt) fire_halo_piece(hp, hpp, (ccc & 1) ^ 1);
    }
    // keep the MFMAs below the DMA launch: without this the compiler hoists all of them above it (they do not
    // depend on it) and the loads start ~24 MFMA issue slots later
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) asm volatile("" : "+v"(acc[i][j]));
    // (on the last iteration this reads a stale buffer into registers nobody uses)
    if constexpr (HALO) {
      set_tap(ctap);
      read_frag(f0, smem + (ccc & 1) * T::STAGE, smem + nbuf * T::STAGE + b_off, 0);
    } else {
      read_frag(f0, smem + nbuf * T::STAGE + a_off, smem + nbuf * T::STAGE + b_off, 0);
    }
    mfma_frag(f1);                                     // last step
    if constexpr (T::BLOCKED) {
      if ((kc & (T::FLUSH - 1)) == T::FLUSH - 1) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            tot[i][j] += acc[i][j];
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
          }
      }
    }
    buf = nbuf;
  }
  conv_dma_landed_barrier();                                // LDS is reused by the epilogue (and the tail DMAs of zeros are in)
  if constexpr (T::BLOCKED) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] += tot[i][j];
  }

  // ---- image layer folded into this layer's epilogue (ConvArgs::img_part)
  if constexpr (BREG && EPI == EPI_MUL && PREC == PREC_BF16X3 && TM == 2 && TN == 1 && WM == 2 && WN == 2) {
    if (a.img_part) {
      static_assert(2 * T::STAGE >= 128 * 64, "the C tile (then S_1 as pairs, in place; then T) inside the staging LDS");
      constexpr int TS2 = 57;                             // T row stride (54 used; odd: conflict-free column reads)
      float* Cs = smem;                                   // [128 rows][64] fp32 — rewritten IN PLACE as S_1's bf16 pairs:
      // row r keeps its 256 B = [chunk 0 | chunk 1] x 128 B, 16 B slots XOR-swizzled with (r >> 1) & 7 like an A tile.  The eight
      // lanes that own a row are neighbours in one wave and LDS serves a wave's instructions in order, so all of a row's
      // reads are done before any of its writes.
      const float inv_tw2 = 1.0f / (float)a.tw;
      // everything this epilogue needs from global memory is requested up front — the gates of this thread's four
      // (row, channel group) items and this wave's fragments of the tap matrix — so that the latencies overlap each other
      // and the LDS passes below instead of sitting between them
      f32x4 gq[4][2];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int item = tid + k * T::NT, row = item >> 3, g = item & 7;
        int ty, tx;
        conv_divmod(row, a.tw, inv_tw2, ty, tx);
        const int Y = Y0 + ty, w = x0 + tx;
        const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
        gq[k][0] = gq[k][1] = z4;                         // (gate = 0 for padding rows / pixels outside the image)
        if (row < a.th * a.tw && Y < yend && w < a.W) {
          int n, h;
          conv_divmod(Y, a.H, inv_H, n, h);
          const int img = a.row2img ? a.row2img[n] : n;
          const float* gp = a.aux + ((size_t)img * HW + h * a.W + w) * a.N + g * 8;
          gq[k][0] = *reinterpret_cast<const f32x4*>(gp); gq[k][1] = *reinterpret_cast<const f32x4*>(gp + 4);
        }
      }
      u32x4 wq[2][2][2][2];                               // [chunk][step][hi|lo][n tile]
      {
        const int h2 = lane >> 5;
#pragma unroll
        for (int cc = 0; cc < 2; ++cc)
#pragma unroll
          for (int st = 0; st < 2; ++st)
#pragma unroll
            for (int hl = 0; hl < 2; ++hl)
#pragma unroll
              for (int j = 0; j < 2; ++j)
                wq[cc][st][hl][j] = *reinterpret_cast<const u32x4*>(a.img_w + (size_t)(j * 32 + (lane & 31)) * 64 + cc * 32 + (4 * st + 2 * h2 + hl) * 4);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          Cs[((wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * 64 + wn * 32 + (lane & 31)] = acc[i][0][r];
      __syncthreads();
#pragma unroll
      for (int k = 0; k < 4; ++k) {                       // 128 rows x 8 channel groups = 1024 items over 256 threads
        const int item = tid + k * T::NT, row = item >> 3, g = item & 7;
        float* rp = Cs + row * 64 + (g >> 2) * 32;
        const f32x4 c0 = *reinterpret_cast<const f32x4*>(rp + (g & 3) * 8), c1 = *reinterpret_cast<const f32x4*>(rp + (g & 3) * 8 + 4);
        float v[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[e] = c0[e] * gq[k][0][e]; v[4 + e] = c1[e] * gq[k][1][e]; }
        bf16x8 hi, lo;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          hi[q] = (__bf16)v[q];
          lo[q] = (__bf16)(v[q] - (float)hi[q]);
        }
        const int d = ((2 * (g & 3)) ^ ((row >> 1) & 7)) << 2;
        *reinterpret_cast<u32x4*>(rp + d) = __builtin_bit_cast(u32x4, hi);
        *reinterpret_cast<u32x4*>(rp + (d ^ 4)) = __builtin_bit_cast(u32x4, lo);
      }
      __syncthreads();
      // T = S_1 . W: wave w owns tile rows 32 w .. 32 w + 31, all 64 columns; K = 64 = 2 chunks x 2 steps
      f32x16 t2[2];
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) t2[j][r] = 0.f;
      {
        const int a_row = wave * 32 + (lane & 31), swz2 = (lane >> 1) & 7, h2 = lane >> 5;
#pragma unroll
        for (int cc = 0; cc < 2; ++cc)
#pragma unroll
          for (int st = 0; st < 2; ++st) {
            const bf16x8 ah = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(Cs + a_row * 64 + cc * 32 + (((4 * st + 2 * h2) ^ swz2) << 2)));
            const bf16x8 al = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(Cs + a_row * 64 + cc * 32 + (((4 * st + 2 * h2 + 1) ^ swz2) << 2)));
#pragma unroll
            for (int j = 0; j < 2; ++j) {
              const bf16x8 bh = __builtin_bit_cast(bf16x8, wq[cc][st][0][j]), bl = __builtin_bit_cast(bf16x8, wq[cc][st][1][j]);
              t2[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, t2[j], 0, 0, 0);
              t2[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, t2[j], 0, 0, 0);
              t2[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, t2[j], 0, 0, 0);
            }
          }
      }
      __syncthreads();                                    // every wave is done reading A2: T may overwrite it
      float* Ts = smem;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int lr = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int col = j * 32 + (lane & 31);
          if (col < TS2) Ts[lr * TS2 + col] = t2[j][r];
        }
      }
      __syncthreads();
      // partial sums of the ring-inclusive positions: output (oy, ox) in [-1, th] x [-1, tw] tile coordinates gets
      // sum over taps of T[source = (oy - (kh - 1), ox - (kw - 1))][tap] for the sources this tile owns
      const int RW = a.tw + 2, npos = (a.th + 2) * RW;
      const int mtp_ = a.tile_map ? a.tile_map[mt] : mt;
      for (int p = tid; p < npos; p += T::NT) {
        const int ry = p / RW, rx = p - ry * RW, oy = ry - 1, ox = rx - 1;
        float pos[3] = {0.f, 0.f, 0.f}, neg[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          const int sy = oy - (tap / 3 - 1), sx = ox - (tap % 3 - 1);
          if (sy >= 0 && sy < a.th && sx >= 0 && sx < a.tw && Y0 + sy < yend && x0 + sx < a.W) {
            const float* r = Ts + (sy * a.tw + sx) * TS2 + tap * 6;
            pos[0] += r[0]; pos[1] += r[1]; pos[2] += r[2];
            neg[0] += r[3]; neg[1] += r[4]; neg[2] += r[5];
          }
        }
        float* o = a.img_part + ((size_t)mtp_ * npos + p) * 6;
        o[0] = pos[0]; o[1] = pos[1]; o[2] = pos[2]; o[3] = neg[0]; o[4] = neg[1]; o[5] = neg[2];
      }
      return;
    }
  }

  // ---- conv-LRP epilogues: stage the C tile through the (now idle) LDS so that the gate loads
  // and the relevance stores are 16 B per lane along the channel axis (a pixel's channels are
  // contiguous in NHWC) instead of one dword per lane.
  if constexpr (EPI == EPI_IMG_STENCIL) {
    // row stride 65 floats: with 64 (= 256 B = one sweep of the banks) the stencil's reads of one column across the
    // 64 pixels of a wave all hit the same bank  [MI355X: SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.75]
    constexpr int TS = T::BN + 1;
    static_assert(T::BM == IMG_PATCH * IMG_PATCH && T::BN == 64 && T::BM * TS <= 2 * T::STAGE, "patch tile is 256 x 64");
    float* Ts = smem;                                   // T of the patch: [256 patch pixels][64 columns (54 used)]
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int lr = (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
#pragma unroll
        for (int j = 0; j < TN; ++j) Ts[lr * TS + (wn * TN + j) * 32 + (lane & 31)] = acc[i][j][r];
      }
    __syncthreads();
    // R_img[p] = sum_tap T[p - d(tap)][tap], d = (kh - 1, kw - 1): patch pixel (oy + 2 - kh, ox + 2 - kw)
    for (int o = tid; o < IMG_TILE * IMG_TILE; o += T::NT) {
      const int oy = o / IMG_TILE, ox = o - oy * IMG_TILE;
      const int y = py0 + oy, x = px0 + ox;
      if (y >= a.H || x >= a.W) continue;
      float pos[3] = {0.f, 0.f, 0.f}, neg[3] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const float* r = Ts + ((oy + 2 - tap / 3) * IMG_PATCH + (ox + 2 - tap % 3)) * TS + tap * 6;
        pos[0] += r[0]; pos[1] += r[1]; pos[2] += r[2];
        neg[0] += r[3]; neg[1] += r[4]; neg[2] += r[5];
      }
      const int img = a.row2img ? a.row2img[pn] : pn;
      if constexpr (PREC == PREC_F16X2) {               // undo the token's scale: the chain ends here
        const float sc = a.tok_fac[pn];
#pragma unroll
        for (int c = 0; c < 3; ++c) { pos[c] *= sc; neg[c] *= sc; }
      }
      const float* xv = a.ximg + ((size_t)img * HW + (size_t)y * a.W + x) * 3;
      float* ov = a.out + ((size_t)pn * HW + (size_t)y * a.W + x) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (a.img_mode == 0) ov[c] = xv[c] >= 0.f ? xv[c] * pos[c] : xv[c] * neg[c];   // LRP alpha1beta0 at the image
        else if (a.img_mode == 1) ov[c] = pos[c] + neg[c];                                // plain gradient
        else if (a.img_mode == 2) ov[c] = xv[c] * (pos[c] + neg[c]);                      // input x gradient
        else ov[c] = (xv[c] - a.img_lo) * pos[c] + (xv[c] - a.img_hi) * neg[c];           // BoundedRule (RR:430-439)
      }
    }
    return;
  } else if constexpr (EPI != EPI_STORE) {
    // The C tile goes through the staging LDS in NH row slabs (a 256-row tile does not fit at once).
    float* Cs = smem;
    const int c4 = tid % T::C4, rin = tid / T::C4;
    const int col = n0 + c4 * T::CW;
    const int tn0 = m0 / HW, tp0 = m0 - tn0 * HW;
    const float invw = 1.0f / (float)a.W;
    // tile row lr -> linear NHWC row / image slot n / pixel (h, w); false = padding row
    auto locate = [&](int lr, int& row, int& n, int& h, int& w) -> bool {
      if constexpr (HALO) {
        int ty, tx;
        conv_divmod(lr, a.tw, inv_tw, ty, tx);
        const int Y = Y0 + ty;
        w = x0 + tx;
        if (lr >= a.th * a.tw || Y >= yend || w >= a.W) return false;
        conv_divmod(Y, a.H, inv_H, n, h);
        row = Y * a.W + w;
        return true;
      } else {
        row = m0 + lr;
        if (row >= a.M) return false;
        if constexpr (EPI == EPI_MUL || EPI == EPI_MUL_UP2) {
          n = tn0;
          int pix = tp0 + lr;
          while (pix >= HW) { pix -= HW; ++n; }
          h = (int)(((float)pix + 0.5f) * invw);
          w = pix - h * a.W;
          if (w < 0) { --h; w += a.W; } else if (w >= a.W) { ++h; w -= a.W; }
        }
        return true;
      }
    };
    // PREC_F16X2: largest |stored output| per token, gathered per block in LDS (slot = token - first token of the tile) and
    // flushed with ONE global atomic per token and block (a global atomic per wave and pass cost 0.4 ms on block1_conv2)
    // (the slots live in the staging LDS behind the C slab where the tile shape leaves room — every tile does except the
    // non-halo 128 x 128 / 256 x 256 ones, which fall back to the per-wave global atomic; LDS is sized to the byte:
    // two 128 x 128 halo blocks fill the CU's 160 KB exactly)
    unsigned* tmax_s = reinterpret_cast<unsigned*>(smem + T::RH * T::BN);
    const int tok_first = HALO ? img0 : tn0;
    if constexpr (T::TMAX_LDS) {
      if (tid < 16) tmax_s[tid] = 0u;                   // (ordered before its first use by the barrier that publishes the C slab)
    }
#pragma unroll 1
    for (int hf = 0; hf < T::NH; ++hf) {
      if (hf) __syncthreads();                          // previous slab fully consumed
      if ((wm * TM * 32) / T::RH == hf) {
        // a wave's TM x 32 rows lie inside ONE slab (static_assert above), so their position in the slab does not depend on hf:
        // one base address + compile-time offsets (written with `- hf * RH` hipcc kept sixteen addresses per wave alive across
        // the main loop of the 8-wave tile, spilled them, and reloaded each behind its own s_waitcnt vmcnt(0))
        float* cw = Cs + (((wm * TM * 32) % T::RH) + 4 * (lane >> 5)) * T::BN + wn * TN * 32 + (lane & 31);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r)
#pragma unroll
            for (int j = 0; j < TN; ++j) cw[(i * 32 + (r & 3) + 8 * (r >> 2)) * T::BN + j * 32] = acc[i][j][r];
      }
      __syncthreads();
      if constexpr (EPI == EPI_BIAS || EPI == EPI_BIAS_RELU) {
        if (col < a.N) {
          const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
          const f32x4 bv = a.bias ? *reinterpret_cast<const f32x4*>(a.bias + col) : zero4;
          float unscale = 1.f;                            // PREC_F16X2: the input's power-of-two scale, undone on the accumulator
          float omax = 0.f;
          if constexpr (PREC == PREC_F16X2) unscale = *a.in_unscale;
#pragma unroll 4
          for (int ps = 0; ps < T::RH / T::RPP; ++ps) {
            const int ll = rin + ps * T::RPP;
            int row, n_, h_, w_;
            if (!locate(hf * T::RH + ll, row, n_, h_, w_)) continue;
            f32x4 v = *reinterpret_cast<const f32x4*>(Cs + ll * T::BN + c4 * 4);
            if constexpr (PREC == PREC_F16X2) v *= unscale;
            v += bv;
            if (a.addend) v += *reinterpret_cast<const f32x4*>(a.addend + (size_t)row * a.N + col);   // second pass of a product
            if constexpr (EPI == EPI_BIAS) {
              if (a.gate_src) {
                const f32x4 av = *reinterpret_cast<const f32x4*>(a.gate_src + (size_t)row * a.N + col);
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = av[q] / (v[q] + (v[q] == 0.f ? 1e-7f : 0.f));
              }
            }
            if constexpr (EPI == EPI_BIAS_RELU) {
#pragma unroll
              for (int q = 0; q < 4; ++q) v[q] = fmaxf(v[q], 0.f);
            }
            if constexpr (PREC == PREC_F16X2) omax = fmaxf(omax, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
            *reinterpret_cast<f32x4*>(a.out + (size_t)row * a.N + col) = v;
          }
          if constexpr (PREC == PREC_F16X2) {
            if (a.act_max_out) {                          // one atomic per wave, spread over ACT_MAX_SLOTS addresses
#pragma unroll
              for (int o = 32; o > 0; o >>= 1) omax = fmaxf(omax, __shfl_xor(omax, o));
              if (lane == 0 && omax > 0.f) atomicMax(a.act_max_out + ((blockIdx.x + wave) & (ACT_MAX_SLOTS - 1)), __float_as_uint(omax));
            }
          }
        }
      } else if constexpr (EPI == EPI_FWD_DUAL) {
        if (a.dual_il) {
          // interleaved columns: tile column p -> block p / 32; even block = c of channels ch.., the odd block behind it =
          // Z+ of the same channels.  The two threads that own a channel quad (one per block) share its rows by parity.
          const int p = c4 * 4, half = (p >> 5) & 1;
          const int ch = (n0 >> 1) + (p >> 6) * 32 + (p & 31);
          bool pooled = false;
          if constexpr (HALO && T::NH == 1 && PREC == PREC_F16X2) {
            if (a.pool_gc) {
              // ---- fused 2x2 max-pool (ConvArgs::pool_gc): item = (window of the tile, channel quad)
              pooled = true;
              const int wpr = a.tw >> 1, nq = T::BN / 8;     // windows per tile row; channel quads of the tile's c columns
              const int nitems = (a.th >> 1) * wpr * nq;
              const float inv_wpr = 1.0f / (float)wpr;
              float pmax0 = 0.f, pmax1 = 0.f;
              for (int it = tid; it < nitems; it += T::NT) {
                const int q = it % nq, win = it / nq;
                int wy, wx;
                conv_divmod(win, wpr, inv_wpr, wy, wx);
                const int cq = 4 * q, chp = (n0 >> 1) + cq, pcp = (cq >> 5) * 64 + (cq & 31);
                const int r00 = (2 * wy) * a.tw + 2 * wx;
                int row = 0, n_ = 0, h_ = 0, w_ = 0;
                const bool ok = locate(r00, row, n_, h_, w_) && chp < a.split;
                const int rel = a.scale_per_img ? n_ - simg0 : 0;
                float unscale = rel == 0 ? us0 : us1, pscale = rel == 0 ? ps0 : ps1;
                if (ok && rel > 1) { unscale = a.in_unscale[simg0 + rel]; pscale = a.pairs_scale[simg0 + rel]; }
                f32x4 bvp = {0.f, 0.f, 0.f, 0.f};
                if (ok) bvp = *reinterpret_cast<const f32x4*>(a.bias + chp);
                f32x4 mx, zx;
                unsigned posw = 0u;
#pragma unroll
                for (int pp = 0; pp < 4; ++pp) {
                  const float* cr = Cs + (r00 + (pp >> 1) * a.tw + (pp & 1)) * T::BN + pcp;
                  f32x4 vc = *reinterpret_cast<const f32x4*>(cr), vz = *reinterpret_cast<const f32x4*>(cr + 32);
                  vc *= unscale; vz *= unscale;
                  vc += bvp; vz += bvp;
#pragma unroll
                  for (int e = 0; e < 4; ++e) {
                    const float av = a.dual_norelu ? vc[e] : fmaxf(vc[e], 0.f);
                    if (pp == 0 || av > mx[e]) {           // first maximum in scan order (what tf.gradients routes to)
                      mx[e] = av; zx[e] = vz[e];
                      posw = (posw & ~(0xFFu << (8 * e))) | ((unsigned)pp << (8 * e));
                    }
                  }
                }
                f32x4 gq;
#pragma unroll
                for (int e = 0; e < 4; ++e) gq[e] = mx[e] / (zx[e] + (zx[e] == 0.f ? 1e-7f : 0.f));
                if (ok) {
                  const size_t po = (((size_t)n_ * (a.H >> 1) + (h_ >> 1)) * (a.W >> 1) + (w_ >> 1)) * a.split + chp;
                  *reinterpret_cast<f32x4*>(a.pool_gc + po) = gq;
                  *reinterpret_cast<unsigned*>(a.pool_pos + po) = posw;
                  if (a.pool_x) *reinterpret_cast<f32x4*>(a.pool_x + po) = mx;
                  const float m4 = fmaxf(fmaxf(fabsf(mx[0]), fabsf(mx[1])), fmaxf(fabsf(mx[2]), fabsf(mx[3])));
                  if (rel == 0) pmax0 = fmaxf(pmax0, m4);
                  else if (rel == 1) pmax1 = fmaxf(pmax1, m4);
                  else if (m4 > 0.f && a.act_max_out) atomicMax(a.act_max_out + (size_t)(simg0 + rel) * ACT_MAX_SLOTS + ((blockIdx.x + wave) & (ACT_MAX_SLOTS - 1)), __float_as_uint(m4));
                }
                {
                  // pairs of the pooled activation: the two lanes of a split8 group (quads q, q ^ 1: neighbouring items of the
                  // same window) swap halves and store 16 B each, as in the unpooled epilogue below
                  typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
                  typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
                  f16x4 hi, lo;
#pragma unroll
                  for (int e = 0; e < 4; ++e) {
                    const float sv = mx[e] * pscale;
                    hi[e] = (_Float16)sv;
                    lo[e] = (_Float16)(sv - (float)hi[e]);
                  }
                  const bool odd = q & 1;
                  const u32x2 mine = __builtin_bit_cast(u32x2, odd ? lo : hi);
                  const u32x2 give = __builtin_bit_cast(u32x2, odd ? hi : lo);
                  u32x2 got;
                  got[0] = __shfl_xor(give[0], 1);
                  got[1] = __shfl_xor(give[1], 1);
                  u32x4 v16;
                  v16[0] = odd ? got[0] : mine[0]; v16[1] = odd ? got[1] : mine[1];
                  v16[2] = odd ? mine[0] : got[0]; v16[3] = odd ? mine[1] : got[1];
                  if (ok) {
                    const size_t po = (((size_t)n_ * (a.H >> 1) + (h_ >> 1)) * (a.W >> 1) + (w_ >> 1)) * a.split + (chp & ~7);
                    *reinterpret_cast<u32x4*>(a.pairs_out + po + (odd ? 4 : 0)) = v16;
                  }
                }
              }
              if (a.act_max_out) {
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                  pmax0 = fmaxf(pmax0, __shfl_xor(pmax0, o));
                  pmax1 = fmaxf(pmax1, __shfl_xor(pmax1, o));
                }
                unsigned* ms = a.act_max_out + (size_t)simg0 * ACT_MAX_SLOTS + ((blockIdx.x + wave) & (ACT_MAX_SLOTS - 1));
                if (lane == 0 && pmax0 > 0.f) atomicMax(ms, __float_as_uint(pmax0));
                if (lane == 0 && pmax1 > 0.f) atomicMax(ms + ACT_MAX_SLOTS, __float_as_uint(pmax1));
              }
            }
          }
          if (!pooled && ch < a.split) {
            const f32x4 bv = *reinterpret_cast<const f32x4*>(a.bias + ch);
            const int pc = (p & ~63) + (p & 31);          // the c column of the pair; Z+ sits 32 further
            // running max|a_l| of this thread's rows of images simg0 .. simg0 + 3 (a tile spans more than two images where an
            // image is a few dozen rows — the 7 x 7 maps of a ResNet's last stack: as unreduced atomics per row those launches
            // took 250 us instead of 36 [MI355X])
            float omax0 = 0.f, omax1 = 0.f, omax2 = 0.f, omax3 = 0.f;
            auto max_slot = [&](int img) { return a.act_max_out + (size_t)img * ACT_MAX_SLOTS + ((blockIdx.x + wave) & (ACT_MAX_SLOTS - 1)); };
            static_assert((T::RH / T::RPP) % 4 == 0, "constant, even trip count: the loop holds lane shuffles (no remainder loop)");
#pragma unroll 2
            for (int pi = 0; pi < T::RH / T::RPP / 2; ++pi) {
              const int ll = rin + (half + 2 * pi) * T::RPP;
              int row, n_, h_, w_;
              if (!locate(hf * T::RH + ll, row, n_, h_, w_)) continue;
              int rimg = 0;                                // image of the row (1-tap launches over a pixel list: rows / image is
              if (a.scale_per_img) {                       //  not a power of two — float estimate + fix-up, not an integer division)
                if constexpr (HALO) rimg = n_;
                else { int rr; conv_divmod(row, a.img_rows, inv_img_rows, rimg, rr); }
              }
              const int rel = rimg - simg0;
              float unscale = rel == 0 ? us0 : us1, pscale = rel == 0 ? ps0 : ps1;
              if (__builtin_expect(rel > 1, 0)) {         // (a tile over three or more images: images smaller than half a tile)
                if constexpr (PREC == PREC_F16X2) unscale = a.in_unscale[simg0 + rel];
                if (a.pairs_out) pscale = a.pairs_scale[simg0 + rel];
              }
              f32x4 vc = *reinterpret_cast<const f32x4*>(Cs + ll * T::BN + pc);
              f32x4 vz = *reinterpret_cast<const f32x4*>(Cs + ll * T::BN + pc + 32);
              if constexpr (PREC == PREC_F16X2) { vc *= unscale; vz *= unscale; }
              vc += bv; vz += bv;
              if (!a.dual_norelu) {
#pragma unroll
                for (int q = 0; q < 4; ++q) vc[q] = fmaxf(vc[q], 0.f);
              }
              if (a.dual_gate == 2) {
                const f32x4 ga = *reinterpret_cast<const f32x4*>(a.bn_gamma + ch), be = *reinterpret_cast<const f32x4*>(a.bn_beta + ch);
                const f32x4 mu = *reinterpret_cast<const f32x4*>(a.bn_mean + ch), va = *reinterpret_cast<const f32x4*>(a.bn_var + ch);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                  const float cv = vc[q];
                  const float y = ga[q] * (cv - mu[q]) / sqrtf(va[q] + a.bn_eps) + be[q];
                  const float d = (cv - mu[q]) * y;
                  const float ds = d + (d >= 0.f ? 1e-7f : -1e-7f);                      // sign stabiliser, then SafeDivide
                  const float qq = (cv * (y - be[q])) / (ds + (ds == 0.f ? 1e-7f : 0.f)) / (vz[q] + (vz[q] == 0.f ? 1e-7f : 0.f));
                  const float av = a.bn_relu ? fmaxf(y, 0.f) : y;
                  vc[q] = av;
                  vz[q] = a.bn_relu ? av * qq : qq;
                }
              } else if (a.dual_gate) {
#pragma unroll
                for (int q = 0; q < 4; ++q) vz[q] = vc[q] / (vz[q] + (vz[q] == 0.f ? 1e-7f : 0.f));
              }
              if (a.act_max_out) {
                const float m4 = fmaxf(fmaxf(fabsf(vc[0]), fabsf(vc[1])), fmaxf(fabsf(vc[2]), fabsf(vc[3])));
                if (rel == 0) omax0 = fmaxf(omax0, m4);
                else if (rel == 1) omax1 = fmaxf(omax1, m4);
                else if (rel == 2) omax2 = fmaxf(omax2, m4);
                else if (rel == 3) omax3 = fmaxf(omax3, m4);
                else if (m4 > 0.f) atomicMax(max_slot(simg0 + rel), __float_as_uint(m4));
              }
              if (!a.skip_out) *reinterpret_cast<f32x4*>(a.out + (size_t)row * a.split + ch) = vc;
              *reinterpret_cast<f32x4*>(a.out2 + (size_t)row * a.split + ch) = vz;
              {
                if (a.pairs_out) {
                  // This thread's 4 channels are one half of a split8 group [8 x fp16 hi | 8 x fp16 lo]; the other half sits
                  // in the neighbouring lane (same row, next channel quad: c4 ^ 1).  The two swap halves so that each issues
                  // ONE 16-byte store (the even lane the group's hi half, the odd lane its lo half) — as 8-byte stores the
                  // epilogue was store-issue-bound [MI355X: the forward convs 8-10 % slower].
                  typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
                  typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
                  f16x4 hi, lo;
#pragma unroll
                  for (int q = 0; q < 4; ++q) {
                    const float sv = vc[q] * pscale;
                    hi[q] = (_Float16)sv;
                    lo[q] = (_Float16)(sv - (float)hi[q]);
                  }
                  const bool odd = (ch >> 2) & 1;
                  const u32x2 mine = __builtin_bit_cast(u32x2, odd ? lo : hi);      // what this lane keeps
                  const u32x2 give = __builtin_bit_cast(u32x2, odd ? hi : lo);      // what the neighbour stores
                  u32x2 got;
                  got[0] = __shfl_xor(give[0], 1);
                  got[1] = __shfl_xor(give[1], 1);
                  u32x4 v16;
                  v16[0] = odd ? got[0] : mine[0]; v16[1] = odd ? got[1] : mine[1];     // channels 0-3 of the group first
                  v16[2] = odd ? mine[0] : got[0]; v16[3] = odd ? mine[1] : got[1];
                  float* grp = a.pairs_out + (size_t)row * a.split + (ch & ~7);
                  *reinterpret_cast<u32x4*>(grp + (odd ? 4 : 0)) = v16;
                }
              }
            }
            if (a.act_max_out) {                            // (any PREC: the image layer's fp32 GEMM raises its maximum here too)
#pragma unroll
              for (int o = 32; o > 0; o >>= 1) {
                omax0 = fmaxf(omax0, __shfl_xor(omax0, o));
                omax1 = fmaxf(omax1, __shfl_xor(omax1, o));
                omax2 = fmaxf(omax2, __shfl_xor(omax2, o));
                omax3 = fmaxf(omax3, __shfl_xor(omax3, o));
              }
              if (lane == 0 && omax0 > 0.f) atomicMax(max_slot(simg0), __float_as_uint(omax0));
              if (lane == 0 && omax1 > 0.f) atomicMax(max_slot(simg0 + 1), __float_as_uint(omax1));
              if (lane == 0 && omax2 > 0.f) atomicMax(max_slot(simg0 + 2), __float_as_uint(omax2));
              if (lane == 0 && omax3 > 0.f) atomicMax(max_slot(simg0 + 3), __float_as_uint(omax3));
            }
          }
        } else
        // cols [0,split) -> out = relu(acc + bias)  (a_l);  cols [split,2 split) -> out2 = acc + bias  (Z+_l)
        if (col < 2 * a.split) {
          const bool isz = col >= a.split;
          const int c = isz ? col - a.split : col;
          const f32x4 bv = *reinterpret_cast<const f32x4*>(a.bias + c);
          float* dst = (isz ? a.out2 : a.out) + c;
          float unscale = 1.f, omax = 0.f;                // PREC_F16X2: as in the BIAS epilogues (max of the a half only)
          if constexpr (PREC == PREC_F16X2) unscale = *a.in_unscale;
#pragma unroll 4
          for (int ps = 0; ps < T::RH / T::RPP; ++ps) {
            const int ll = rin + ps * T::RPP;
            int row, n_, h_, w_;
            if (!locate(hf * T::RH + ll, row, n_, h_, w_)) continue;
            f32x4 v = *reinterpret_cast<const f32x4*>(Cs + ll * T::BN + c4 * 4);
            if constexpr (PREC == PREC_F16X2) v *= unscale;
            v += bv;
            if (!isz && !a.dual_norelu) {
#pragma unroll
              for (int q = 0; q < 4; ++q) v[q] = fmaxf(v[q], 0.f);
            }
            if constexpr (PREC == PREC_F16X2) {
              if (!isz) omax = fmaxf(omax, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
            }
            *reinterpret_cast<f32x4*>(dst + (size_t)row * a.split) = v;
          }
          if constexpr (PREC == PREC_F16X2) {
            if (a.act_max_out) {
#pragma unroll
              for (int o = 32; o > 0; o >>= 1) omax = fmaxf(omax, __shfl_xor(omax, o));
              if (lane == 0 && omax > 0.f) atomicMax(a.act_max_out + ((blockIdx.x + wave) & (ACT_MAX_SLOTS - 1)), __float_as_uint(omax));
            }
          }
        }
      } else {
        // out = acc * gate (fp32), stored as fp32 or re-split into [hi8 | lo8] for the next layer's MFMAs.
        // The gate values are two dependent global loads away (row2img[n], then the gate row) and nothing in a pass
        // depends on the pass before it, so the loads are issued in bulk: every pass's image slot first, then the
        // gate rows one pass AHEAD of the arithmetic (written as explicit phases — left as load/multiply/store per
        // pass, the possible aliasing of `out` and `aux` made hipcc serialise a full memory round trip per pass, which
        // the short K = 576 layers could not hide).
        if (col < a.N) {
          // ---- the walk's common case (plain gate, no residual join, no second head, no gradient-walk switches): the same
          // arithmetic with nothing to decide inside the passes.  In the general form below every runtime switch sits next to
          // a load, hipcc branches around those loads, cannot count them any more and drains the queue (s_waitcnt vmcnt(0) /
          // (1)) in every pass — the gate rows requested "one pass ahead" were in fact waited for immediately, and an 8-wave
          // tile's epilogue ran as 16 dependent L2 round trips with the matrix pipe idle.  Here the gate loads of RING passes
          // are in flight, unconditionally (padding rows read row 0 of image 0), and each pass waits with a counted vmcnt.
          // Rows are located twice (at issue and at use: a few VALU ops) instead of keeping six arrays of NP entries alive.
          // Dual gate (DG, ConvArgs::aux_b): always this form, with a second gate row per pass — one accumulator, two gates, two
          // outputs of ostride floats per pixel — and a shorter ring (two gate sets per entry).
          if constexpr (PREC != PREC_F16X2) {
            const bool tail_ = EPI == EPI_MUL && a.join != nullptr, head2_ = EPI == EPI_MUL && a.out2s != nullptr;
            if (DG || (!GMASK && !(EPI == EPI_MUL && a.gate_none) && !tail_ && !head2_ && !a.gate_binary && !a.relu_out && !a.epi_generic)) {
              constexpr int NPf = T::RH / T::RPP;
              constexpr int UPf = EPI == EPI_MUL_UP2 ? 4 : 1;
              constexpr int NG = DG ? 2 : 1;              // gates per pass; gate b of ring slot s lies in gq[b * RING + s]
              constexpr int DEPTH = DG ? (UPf == 1 ? 2 : 1) : (UPf == 1 ? 4 : 2);
              constexpr int RING = DEPTH < NPf ? DEPTH : NPf;
              const int W2f = 2 * a.W, H2f = 2 * a.H;
              int imgf[NPf];
#pragma unroll
              for (int ps = 0; ps < NPf; ++ps) {
                int row, n_, h_, w_;
                if (!locate(hf * T::RH + rin + ps * T::RPP, row, n_, h_, w_)) n_ = 0;
                imgf[ps] = a.row2img ? a.row2img[n_] : n_;
              }
              f32x4 gq[NG * RING][UPf][T::CW / 4];
              auto issue = [&](int ps) {
                int row, n_, h_, w_;
                if (!locate(hf * T::RH + rin + ps * T::RPP, row, n_, h_, w_)) { h_ = 0; w_ = 0; }
#pragma unroll
                for (int q = 0; q < UPf; ++q) {
                  const float* gp = EPI == EPI_MUL ? a.aux + ((size_t)imgf[ps] * HW + h_ * a.W + w_) * a.N + col
                                                   : a.aux + (((size_t)imgf[ps] * H2f + 2 * h_ + (q >> 1)) * W2f + 2 * w_ + (q & 1)) * a.N + col;
#pragma unroll
                  for (int q4 = 0; q4 < T::CW / 4; ++q4) gq[ps % RING][q][q4] = *reinterpret_cast<const f32x4*>(gp + 4 * q4);
                  if constexpr (DG) {
#pragma unroll
                    for (int q4 = 0; q4 < T::CW / 4; ++q4) gq[RING + ps % RING][q][q4] = *reinterpret_cast<const f32x4*>(a.aux_b + (gp - a.aux) + 4 * q4);
                  }
                }
              };
#pragma unroll
              for (int ps = 0; ps < RING - 1; ++ps) issue(ps);
              const bool plain = T::SPLIT_OUT && a.out_plain;
#pragma unroll
              for (int ps = 0; ps < NPf; ++ps) {
                if (ps + RING - 1 < NPf) issue(ps + RING - 1);
                int row, n_, h_, w_;
                if (locate(hf * T::RH + rin + ps * T::RPP, row, n_, h_, w_)) {
                  const int ll = rin + ps * T::RPP;
                  float v[T::CW];
#pragma unroll
                  for (int q4 = 0; q4 < T::CW / 4; ++q4)
                    *reinterpret_cast<f32x4*>(v + 4 * q4) = *reinterpret_cast<const f32x4*>(Cs + ll * T::BN + c4 * T::CW + 4 * q4);
#pragma unroll
                  for (int q = 0; q < UPf; ++q) {
                    float r[T::CW];
#pragma unroll
                    for (int q4 = 0; q4 < T::CW / 4; ++q4)
#pragma unroll
                      for (int e = 0; e < 4; ++e) r[4 * q4 + e] = v[4 * q4 + e] * gq[ps % RING][q][q4][e];
                    float* dst = EPI == EPI_MUL
                                     ? a.out + (size_t)row * a.N + col
                                     : a.out + (((size_t)n_ * H2f + 2 * h_ + (q >> 1)) * W2f + 2 * w_ + (q & 1)) * a.N + col;
                    if constexpr (DG)                     // out / out_b: ostride floats per pixel
                      dst = a.out + (EPI == EPI_MUL ? (size_t)row : ((size_t)n_ * H2f + 2 * h_ + (q >> 1)) * W2f + 2 * w_ + (q & 1)) * a.ostride + col;
                    if constexpr (T::SPLIT_OUT) {
                      if (plain) {
                        *reinterpret_cast<f32x4*>(dst) = *reinterpret_cast<const f32x4*>(r);
                        *reinterpret_cast<f32x4*>(dst + 4) = *reinterpret_cast<const f32x4*>(r + 4);
                      } else {
                        split8_store(r, dst);
                      }
                    } else {
                      *reinterpret_cast<f32x4*>(dst) = *reinterpret_cast<const f32x4*>(r);
                    }
                    if constexpr (DG) {                   // the same accumulator under the second gate
#pragma unroll
                      for (int q4 = 0; q4 < T::CW / 4; ++q4)
#pragma unroll
                        for (int e = 0; e < 4; ++e) r[4 * q4 + e] = v[4 * q4 + e] * gq[RING + ps % RING][q][q4][e];
                      float* dstb = a.out_b + (dst - a.out);
                      if constexpr (T::SPLIT_OUT) {
                        if (plain) {
                          *reinterpret_cast<f32x4*>(dstb) = *reinterpret_cast<const f32x4*>(r);
                          *reinterpret_cast<f32x4*>(dstb + 4) = *reinterpret_cast<const f32x4*>(r + 4);
                        } else {
                          split8_store(r, dstb);
                        }
                      } else {
                        *reinterpret_cast<f32x4*>(dstb) = *reinterpret_cast<const f32x4*>(r);
                      }
                    }
                  }
                }
              }
              continue;                                   // next slab
            }
            // (A counted-prefetch form of the join + second-head epilogue — the tail of a ResNet identity block — was built here in
            //  round 4: config 4 -0.5 ms, but its mere presence in this instantiation cost the VGG walk's launches 2.4 %
            //  [MI355X, same box: 24.55 -> 25.15 ms, WRITE_SIZE +11 %: the register allocator spilled], so it was taken out
            //  again; those launches are bound by their three full-width streams either way)
          }
          if constexpr (!DG) {                           // the general pass loop: one gate
            constexpr int NP = T::RH / T::RPP;
            constexpr int UPN = EPI == EPI_MUL_UP2 ? 4 : 1;
            const int W2 = 2 * a.W, H2 = 2 * a.H;
            int rowv[NP], nv[NP], hv[NP], wv[NP], imgv[NP];
            bool okv[NP];
#pragma unroll
            for (int ps = 0; ps < NP; ++ps) {
              okv[ps] = locate(hf * T::RH + rin + ps * T::RPP, rowv[ps], nv[ps], hv[ps], wv[ps]);
              if (!okv[ps]) { rowv[ps] = 0; nv[ps] = 0; hv[ps] = 0; wv[ps] = 0; }
              imgv[ps] = a.row2img ? a.row2img[nv[ps]] : nv[ps];
            }
            // PREC_F16X2: running maximum of |stored output| for the token of the rows this thread has seen so far
            unsigned lmax = 0u;
            int ltok = -1;
            auto flush_max = [&](int t, unsigned m) {
              if (m) {
                const int rel = t - tok_first;
                if (T::TMAX_LDS && rel >= 0 && rel < 16) atomicMax(tmax_s + rel, m);
                else atomicMax(a.tok_max_out + t, m);
              }
            };
            const bool tail = EPI == EPI_MUL && a.join != nullptr, head2 = EPI == EPI_MUL && a.out2s != nullptr;
            struct Gates { f32x4 g[UPN][T::CW / 4]; f32x4 jn[T::CW / 4], jg[T::CW / 4], g2[T::CW / 4]; };
            auto gate_ptr = [&](int ps, int q) -> const float* {
              if constexpr (EPI == EPI_MUL)
                return a.aux + ((size_t)imgv[ps] * HW + hv[ps] * a.W + wv[ps]) * a.N + col;
              else
                return a.aux + (((size_t)imgv[ps] * H2 + 2 * hv[ps] + (q >> 1)) * W2 + 2 * wv[ps] + (q & 1)) * a.N + col;
            };
            auto load_gates = [&](Gates& G, int ps) {
              const f32x4 one4 = {1.f, 1.f, 1.f, 1.f};
              if constexpr (GMASK) {
                static_assert(EPI == EPI_MUL && PREC == PREC_FP32 && T::CW == 4, "byte-mask gates: exact fp32 EPI_MUL only");
                auto m4 = [](const float* base, size_t e) {
                  const unsigned m = *reinterpret_cast<const unsigned*>(reinterpret_cast<const unsigned char*>(base) + e);
                  f32x4 g;
#pragma unroll
                  for (int q = 0; q < 4; ++q) g[q] = ((m >> (8 * q)) & 0xFFu) ? 1.f : 0.f;
                  return g;
                };
                const size_t go = ((size_t)imgv[ps] * HW + hv[ps] * a.W + wv[ps]) * a.N + col;
                G.g[0][0] = m4(a.aux, go);
                if (tail) {
                  G.jn[0] = *reinterpret_cast<const f32x4*>(a.join + (size_t)rowv[ps] * a.N + col);
                  G.jg[0] = m4(a.join_gate, go);
                }
                return;
              }
#pragma unroll
              for (int q = 0; q < UPN; ++q)
#pragma unroll
                for (int q4 = 0; q4 < T::CW / 4; ++q4)
                  G.g[q][q4] = (EPI == EPI_MUL && a.gate_none) ? one4 : *reinterpret_cast<const f32x4*>(gate_ptr(ps, q) + 4 * q4);
              if constexpr (EPI == EPI_MUL) {
                const size_t go = ((size_t)imgv[ps] * HW + hv[ps] * a.W + wv[ps]) * a.N + col;
#pragma unroll
                for (int q4 = 0; q4 < T::CW / 4; ++q4) {
                  if (tail) {
                    G.jn[q4] = *reinterpret_cast<const f32x4*>(a.join + (size_t)rowv[ps] * a.N + col + 4 * q4);
                    G.jg[q4] = *reinterpret_cast<const f32x4*>(a.join_gate + go + 4 * q4);
                  }
                  if (head2) G.g2[q4] = *reinterpret_cast<const f32x4*>(a.gate2 + go + 4 * q4);
                }
              }
            };
            Gates cur, nxt;
            load_gates(cur, 0);
#pragma unroll
            for (int ps = 0; ps < NP; ++ps) {
              if (ps + 1 < NP) load_gates(nxt, ps + 1);
              float fac16 = 1.f;                            // PREC_F16X2: the power of two this launch adds to the token's scale
              if constexpr (PREC == PREC_F16X2) {
                fac16 = a.tok_fac[nv[ps]];
                if (okv[ps] && nv[ps] != ltok) { flush_max(ltok, lmax); ltok = nv[ps]; lmax = 0u; }
              }
              if (okv[ps]) {
                const int ll = rin + ps * T::RPP;
                float v[T::CW];
#pragma unroll
                for (int q4 = 0; q4 < T::CW / 4; ++q4)
                  *reinterpret_cast<f32x4*>(v + 4 * q4) = *reinterpret_cast<const f32x4*>(Cs + ll * T::BN + c4 * T::CW + 4 * q4);
#pragma unroll
                for (int q = 0; q < UPN; ++q) {
                  float r[T::CW];
#pragma unroll
                  for (int q4 = 0; q4 < T::CW / 4; ++q4) {
                    f32x4 g = cur.g[q][q4];
                    if (a.gate_binary) {
#pragma unroll
                      for (int e = 0; e < 4; ++e) g[e] = g[e] != 0.f ? 1.f : 0.f;
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                      float pr = v[4 * q4 + e] * g[e];
                      if (tail) pr += cur.jn[q4][e] * cur.jg[q4][e];
                      if constexpr (PREC == PREC_F16X2) {
                        pr *= fac16;
                        lmax = max(lmax, __float_as_uint(fabsf(pr)));               // (non-negative floats order like their bits)
                      }
                      r[4 * q4 + e] = a.relu_out ? fmaxf(pr, 0.f) : pr;
                    }
                  }
                  float* dst = EPI == EPI_MUL
                                   ? a.out + (size_t)rowv[ps] * a.N + col
                                   : a.out + (((size_t)nv[ps] * H2 + 2 * hv[ps] + (q >> 1)) * W2 + 2 * wv[ps] + (q & 1)) * a.N + col;
                  if constexpr (T::SPLIT_OUT) {
                    if (a.out_plain) {
                      *reinterpret_cast<f32x4*>(dst) = *reinterpret_cast<const f32x4*>(r);
                      *reinterpret_cast<f32x4*>(dst + 4) = *reinterpret_cast<const f32x4*>(r + 4);
                    } else if constexpr (PREC == PREC_F16X2) {
                      split8h_store(r, dst);
                    } else {
                      split8_store(r, dst);
                    }
                  } else {
                    *reinterpret_cast<f32x4*>(dst) = *reinterpret_cast<const f32x4*>(r);
                  }
                  if (head2) {
                    float r2[T::CW];
#pragma unroll
                    for (int q4 = 0; q4 < T::CW / 4; ++q4)
#pragma unroll
                      for (int e = 0; e < 4; ++e) r2[4 * q4 + e] = r[4 * q4 + e] * cur.g2[q4][e];
                    float* d2 = a.out2s + (size_t)rowv[ps] * a.N + col;
                    if constexpr (T::SPLIT_OUT) {
                      split8_store(r2, d2);
                    } else {
                      *reinterpret_cast<f32x4*>(d2) = *reinterpret_cast<const f32x4*>(r2);
                    }
                  }
                }
              }
              cur = nxt;
            }
            if constexpr (PREC == PREC_F16X2) flush_max(ltok, lmax);
          }
        }
      }
    }
    if constexpr (T::TMAX_LDS && (EPI == EPI_MUL || EPI == EPI_MUL_UP2)) {
      __syncthreads();
      if (tid < 16 && tmax_s[tid]) atomicMax(a.tok_max_out + tok_first + tid, tmax_s[tid]);
    }
    return;
  }

  // ---- scalar epilogue (EPI_STORE, N = 54 is not a multiple of 4).  C/D map of the 32x32 MFMA:
  // col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
  const int col_base = n0 + wn * TN * 32 + (lane & 31);
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = m0 + (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      const bool rv = row < a.M;
      if constexpr (EPI == EPI_STORE) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int col = col_base + j * 32;
          if (rv && col < a.N) a.out[(size_t)row * a.N + col] = acc[i][j][r];
        }
      }
    }
  }
#endif
}

}  // namespace lrp
