// Every conv_igemm_kernel instantiation that is built, and nothing the launch rule (conv_route.hip y2_conv_route) cannot name.  One row per tile
// configuration; its last two columns say which instantiations of it exist.  conv_igemm.hip expands the rows into its table of lines (y2_igemm_line:
// the launcher and what the rule reads of the line's LDS / tile plan).  A route whose tuple is not built is an internal error (YOLO2_E_LAUNCH), never
// another kernel; tests/test_conv_route_cpu.py checks that the recorded shapes of tests/golden/conv_plans.json reach every instantiation.
//   ROW(BM, BN, WGN, stages, split, ctail, chunks, waves, kernel sizes, BN-backward twins)
//   split: 0 = whole tiles, 1 = K-sliced (f32 atomics into the workspace + splitk_finish_kernel), 2 = stream-K
//   kernel sizes: K31 = 3x3 and 1x1, K3 = 3x3 only.  Every row is built for f32 and bf16.
//   twins: the instantiation whose epilogue also reduces the producer layer's BN-backward sums (yolo2_conv2d_dgrad_bn) -- BOTH dtypes, BF16 only, or
//   NONE.  Only whole-channel-row (ctail 0), unsliced instantiations whose wide-store images fit the DMA ring (Y2IgemmPlan::WIDE_FITS) have that
//   form: the K-sliced tiles and, in f32, the 2-stage and the 64-byte-row 128 x 128 rings do not, and the rule sends those to the two-step reduction.
#pragma once
#define Y2_IGEMM_TABLE(ROW)                                                                                \
    ROW(256, 128, 2, 3, 2, 0, 8, 8, K31, BOTH)      /* 256 x 128 stream-K, 8 waves of 64 x 64 */           \
    ROW(128, 128, 2, 3, 2, 0, 8, 8, K31, BOTH)      /* 128 x 128 stream-K, 128-byte rows */                \
    ROW(128, 128, 2, 3, 1, 0, 4, 4, K31, NONE)      /* K-sliced: 4 waves, 64-byte rows */                  \
    ROW(128, 128, 2, 3, 1, 1, 4, 4, K31, NONE)      /* ... with a channel tail */                          \
    ROW(128, 128, 2, 3, 0, 0, 8, 8, K31, BOTH)      /* wide: whole tiles, 128-byte rows, 3 stages */       \
    ROW(128, 128, 2, 2, 0, 0, 8, 8, K31, BF16)      /* full grids: 128-byte rows on a 2-stage ring */      \
    ROW(128, 128, 2, 3, 0, 0, 4, 8, K31, BF16)      /* 8 waves, 64-byte rows (channels no multiple of a 128-byte row) */ \
    ROW(128, 128, 2, 3, 0, 1, 4, 8, K31, NONE)      /* ... with a channel tail */                          \
    ROW(128, 64, 1, 2, 0, 0, 8, 4, K3, BOTH)        /* <= 64 filters, 3x3, 128-byte rows on a 2-stage ring */ \
    ROW(128, 32, 1, 2, 0, 0, 8, 4, K3, BOTH)                                                               \
    ROW(128, 64, 1, 3, 0, 0, 4, 4, K31, BOTH)       /* <= 64 filters, 64-byte rows */                      \
    ROW(128, 64, 1, 3, 0, 1, 4, 4, K31, NONE)                                                              \
    ROW(128, 32, 1, 3, 0, 0, 4, 4, K31, BOTH)                                                              \
    ROW(128, 32, 1, 3, 0, 1, 4, 4, K31, NONE)
