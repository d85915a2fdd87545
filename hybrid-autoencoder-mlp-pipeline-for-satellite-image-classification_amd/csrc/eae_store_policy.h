// Cache policy of the OUTPUT stores, one constant per store family (the `aux` operand of the raw buffer stores of OutRsrc,
// eae_common.hip.h):   0 = plain store (the line is left dirty in the XCD's L2 and written back at the end of the kernel)
//                     16 = write-through (sc1: the line goes to the fabric when it is stored)
// Each can be overridden on the compiler's command line (-DEAE_WT_EPI=0 ...: tools/build_variant.sh + tools/ab.py A/B one family at
// a time).  The policy is no template parameter of a kernel: the kernel names stay what the profiles and profile_hooks key on.
// A family is write-through only where its own A/B showed a gain.  The numbers: ms per step at B=512, mean of six interleaved rounds
// on one box; parent commit 0.4727 (round-to-round spread 0.0035), every family plain 0.4674.
#pragma once

// EPI: TileEpilogue::rows / rows_pre -- every activation and masked gradient of the chain (igemm, igemm2, igemm8, the fc epilogues,
// edge_conv); a wave's store instruction covers whole 128-byte lines.       write-through 0.4564 vs 0.4674 plain: kept
#ifndef EAE_WT_EPI
#define EAE_WT_EPI 16
#endif
// EDGE: deconv4_loss (g4, x_hat, loss partials), edge_wgrad (partials) and its slice reduction (reduce_slices_tall).
//                                                                            write-through 0.4682 vs 0.4674 plain: not kept
#ifndef EAE_WT_EDGE
#define EAE_WT_EDGE 0
#endif
// PART: fp32 partials and their reductions (fc_nt FCE_PARTIAL, fc_splitk_reduce, wgrad_s2, reduce_slices, head, loss_finalize).
//                                                                            write-through 0.4669 vs 0.4674 plain (inside the spread): not kept
#ifndef EAE_WT_PART
#define EAE_WT_PART 0
#endif
// OPT: adam (P, M, V, cleared accumulators) and pack_all.                    write-through 0.4694 vs 0.4674 plain: not kept
// (all four write-through: 0.4566, the EPI figure)
#ifndef EAE_WT_OPT
#define EAE_WT_OPT 0
#endif
// ZONAL: zonal_paint (eae_zonal.hip), an output-only pass outside the training step: a wave's two 16-byte stores per lane cover whole
// 128-byte lines of an int64 raster that nothing in the launch reads back.  Write-through like EPI, the family of the same shape
// (tools/zonal_bench.py times the pass; -DEAE_WT_ZONAL=0 builds the plain form, which was not measured).
#ifndef EAE_WT_ZONAL
#define EAE_WT_ZONAL 16
#endif
// SLIC: the label store of slic_step (eae_slic.hip), written by the last iteration only: a wave's 64 four-byte stores cover 256
// consecutive bytes of an int32 raster that nothing in the launch reads back.  Write-through like ZONAL, the family of the same shape
// (tools/slic_bench.py times the pass; -DEAE_WT_SLIC=0 builds the plain form, which was not measured).
#ifndef EAE_WT_SLIC
#define EAE_WT_SLIC 16
#endif
