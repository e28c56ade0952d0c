// conv_tile.h — what one instantiation of conv_igemm_kernel is made of, and the few pieces of its body that stand on their own.
//   ConvKernelTraits: the kernel's template axes and every tile constant derived from them (waves, tile and piece sizes, LDS
//                     stages and their sum, the epilogue's slabs), with the assertions that constrain them — the kernel reads them
//                     here, and so can anything that wants to know an instantiation's LDS or slab size.
//   the two DMA barriers: what the kernel's loops share and what needs none of the kernel's local state.
// The axes themselves are described above the kernel (conv_igemm.h).  Everything here compiles to the bytes the kernel had with
// these pieces written out in its body.  What does not — the per-block state as a struct, the loops, the epilogues and even
// mfma_frag and the fold of the blocked sum as functions, the LDS array outside the kernel, the folded pair store — was tried, changes registers, scratch or
// speed of some instantiation, and is not here: profiles/conv_kernel_split_ab.txt.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "conv_args.h"
#include "conv_plan.h"

namespace lrp {

// waves per SIMD the register allocator must leave room for: LDS already limits a CU to
// floor(160 KB / LDS per block) blocks of NW waves
constexpr int conv_min_waves(int NW, int TM, int TN, bool halo = false) { return NW == 8 || halo ? 2 : (TM * TN >= 4 ? 2 : 3); }

template <int WM_, int WN_, int TM_, int TN_, int EPI_, int PREC_, bool HALO_, bool BREG_, int TERMS_, int NS_, bool GMASK_, bool PW_, bool DG_, bool C2_ = false>
struct ConvKernelTraits {
  static constexpr int WM = WM_, WN = WN_, TM = TM_, TN = TN_, EPI = EPI_, PREC = PREC_, TERMS = TERMS_, NS = NS_;
  static constexpr bool HALO = HALO_, BREG = BREG_, GMASK = GMASK_, PW = PW_, DG = DG_, C2 = C2_;

  static constexpr int NW = WM * WN, NT = 64 * NW;           // waves / threads per block (4 or 8 waves)
  static constexpr bool SPLIT = PREC != PREC_FP32;            // operands in split8 form (bf16 or fp16 pairs): 16 k per MFMA
  static constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
  static constexpr int AP = BM / 8 / NW, BP = BN / 8 / NW;   // 1 KiB (8-row) DMA pieces per wave and chunk
  static constexpr int HR = conv_halo_rows(BM);              // HALO: LDS rows (pixels) of the resident image
  static constexpr int ABUF = (HALO ? HR : BM) * LDS_STRIDE;
  static constexpr int STAGE = ABUF + (BREG ? 0 : BN) * LDS_STRIDE;
  static constexpr bool BREG8 = BREG && NW == 8;              // the 8-wave 256 x 256 tile with its weights in registers (the kernel's first loop)
  static constexpr bool BREG4 = BREG && NW == 4 && TN == 2;   // the same loop on the 4-wave 128 x 128 tile (FORM_BREG4: walk and dual forward)
  static constexpr bool BREG2 = BREG && NW == 4 && TN == 1 && C2;   // the same loop on the 4-wave 128 x 64 tile (FORM_BREG under LRP_CONV_BREG2: the walk's N <= 64 launches)
  static constexpr bool BREGC = BREG8 || BREG4 || BREG2;      // weights in registers, one barrier per channel CHUNK
  static_assert(!C2 || BREG2, "C2: the chunk loop of the 128 x 64 weights-in-registers tile");
  static_assert(!BREG || (HALO && SPLIT && (BREGC || BM * BN <= 2 * STAGE)), "BREG needs the resident image");
  // which tiles, forms and epilogues go together — BREG8 / BREG4 / BREG2: the dense split-bf16 walk (and, BREG4, the fp16-pair dual forward);
  // PW: that walk on the BREG4 / BREG2 loop; DG: the MUL epilogues of the 4-wave staged / pipelined tiles — is conv_plan.h's table
  static_assert(conv_kernel_instantiated(WM, WN, TM, TN, HALO, BREG, NS, PW, EPI, PREC, TERMS, GMASK, DG, C2), "no such instantiation: conv_plan.h conv_kernel_exists");
  static_assert((BM / 8) % NW == 0 && (BN / 8) % NW == 0, "pieces must divide over the waves");
  static_assert(!HALO || EPI != EPI_STORE, "the image layer is a 1-tap GEMM");
  static_assert(NS == 2 || (NS > 2 && !HALO && !BREG), "deeper staging exists for the plain (non-resident) A path only");
  static constexpr int DPC = AP + BP;                         // DMA instructions per wave and chunk (plain staging)
  static_assert((NS - 2) * DPC <= 63, "vmcnt is a 6-bit counter");
  // BREG8: no B stage, so LDS is the two resident images or one 128-row C slab of the epilogue, whichever is larger (128 KB)
  // BREG4: the two resident images + a spare slot per wave (52 KB) or the epilogue's whole 128 x 128 C tile (64 KB; 80 KB pipelined)
  // BREG2: the same 52 KB (the 128 x 64 C tile is 32 KB): three workgroups per CU
  static constexpr int SMEM = BREG8   ? (2 * STAGE > BM / 2 * BN ? 2 * STAGE : BM / 2 * BN)
                              : BREG4 || BREG2 ? (2 * STAGE + NW * 8 * LDS_STRIDE > BM * BN ? 2 * STAGE + NW * 8 * LDS_STRIDE : BM * BN)
                                      : NS * STAGE;
  static constexpr int CSLAB = BREGC ? SMEM : 2 * STAGE;      // floats the epilogue's C slab may take

  // ---- main loops
  // k steps per 32-wide chunk — fp32: 4 steps of 8 k; split operands: 2 steps of 16 k
  static constexpr int NSTEP = SPLIT ? 2 : 4;
  static_assert(!BREG || NSTEP == 2, "weights in registers: split operands");
  static_assert(!BREGC || SMEM >= 2 * STAGE + NW * 8 * LDS_STRIDE, "a spare LDS slot per wave behind the two images");
  static_assert(!BREGC || 6 * NW * 8 >= HR, "six piece slots per wave cover the resident image");
  // Two-level (blocked) summation: every FLUSH chunks (256 k) the running block is folded into a second accumulator.
  static constexpr int FLUSH = 8;
  // (the fp16-pair forward, whose three-term product is fp32-grade, is blocked as well: without the second level its
  //  accumulator's 3 x K/16 roundings would be the largest error left)
  static constexpr bool BLOCKED = PREC == PREC_FP32 || (PREC == PREC_F16X2 && (EPI == EPI_BIAS || EPI == EPI_BIAS_RELU || EPI == EPI_FWD_DUAL));

  // ---- epilogues
  // The C tile goes through the staging LDS in NH row slabs (a 256-row tile does not fit at once).
  static constexpr bool SLABS = EPI != EPI_STORE && EPI != EPI_IMG_STENCIL;
  static constexpr int NH = (BM * BN + CSLAB - 1) / CSLAB;
  static constexpr int RH = BM / NH;                         // rows per slab
  static_assert(!SLABS || (BM % NH == 0 && RH % (TM * 32) == 0 && RH * BN <= CSLAB), "slab must hold whole wave tiles");
  static constexpr bool SPLIT_OUT = SPLIT && (EPI == EPI_MUL || EPI == EPI_MUL_UP2);
  static constexpr int CW = SPLIT_OUT ? 8 : 4;               // channels per thread (split8 output is written per group)
  static constexpr int C4 = BN / CW, RPP = NT / C4;          // threads along the channels; rows per pass of all threads
  // PREC_F16X2: the per-token maxima of a block are gathered in LDS behind the C slab where the tile shape leaves room (the MUL epilogues)
  static constexpr bool TMAX_LDS = PREC == PREC_F16X2 && RH * BN + 16 <= 2 * STAGE;
};

// hipcc gives __syncthreads() an lgkmcnt(0) only; the LDS-DMA completes on vmcnt, so the wait is explicit
__device__ __forceinline__ void conv_dma_landed_barrier() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}
// NS > 2: the oldest chunk in flight has landed (the NS - 2 younger ones may still be on their way)
template <class T>
__device__ __forceinline__ void conv_dma_oldest_landed_barrier() {
  if constexpr (T::NS > 2) {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((T::NS - 2) * T::DPC) : "memory");
    __syncthreads();
  } else {
    conv_dma_landed_barrier();
  }
}

}  // namespace lrp
