"""The cases of tests/test_plan_edges_gpu.py, (N, H, W, Cin, Cout) unless said otherwise: geometries the plans of the fp16x3
streaming kernels accept and the hourglass's own shapes never produce.  What each is for — on 256 CUs — is asserted by
tests/test_plan_edges_cpu.py.  CONV_F32, at the end: the cases of tests/test_conv_f32_edges_gpu.py, the fp32 family of
csrc/conv_f32.hip across its tile shapes, loaders and K-split chunk counts (no CU count enters its dispatch).  CONV_SPLIT, after
it: the cases of tests/test_conv_split_edges_gpu.py, the tiled split-precision kernels of csrc/conv_split6.hip."""

WGRAD1 = [
    (1, 25, 656, 128, 128),     # 114 slabs x 144 rows = 9 stages (0 mod 3), last slab 128 rows
    (1, 79, 208, 128, 128),     # last slab 16 rows: one stage, shorter than the load pipeline
    (1, 257, 64, 128, 128),     # last slab two stages
    (1, 41, 400, 64, 256),      # two column chunks; share flag: 61 slabs x 17 stages, last 5
    (1, 129, 128, 192, 64),     # three input-channel chunks, 13 stages (1 mod 3), last 5
    (1, 130, 128, 256, 64),     # 128 x 64 tile, two input-channel chunks; share flag: last slab 3 stages
]

GEMM1 = [
    # (case, launched with the share flag)
    ((259, 16, 16, 128, 256), False),   # 259 iterations on 256 workgroups: three run a second one
    ((131, 16, 32, 64, 256), False),    # K = 64, two column chunks, 131 iterations on 128 workgroups
    ((129, 16, 32, 128, 512), False),   # two 256-column chunks, 258 iterations on 128 workgroups
    ((66, 32, 32, 128, 192), True),     # three 64-column chunks; share flag: 66 iterations on 42 workgroups
]

FWD1_ONE_STAGE = [(1, 64, 64, ci, co) for ci, co in
                  [(256, 128), (128, 256), (128, 128), (64, 64), (64, 128), (256, 256)]]       # 4096 rows: one stage per workgroup
FWD1_SHORT_LAST_SHARE = [(1, 43, 96, 256, 128), (1, 43, 96, 64, 64)]      # 129 stages; share flag: two per workgroup, the last has one
                                                                          # (eight-wave 256 -> 128; four-wave 64 -> 64 keeps one each)
FWD1_SHORT_LAST = [(1, 257, 32, 128, 256)]                                # 257 stages: two per workgroup, the last has one
FWD1_DS_STAGES = 129                                                      # the fused conv3 + shortcut launch, 128 -> 256

BWD1_ONE_STAGE = [(1, 128, 128, 64, 64), (1, 128, 128, 64, 128)]          # 16384 rows on four-wave workgroups
BWD1_SHORT_LAST = [(1, 257, 64, 256, 128), (1, 257, 64, 64, 64)]          # 514 stages: 3 per workgroup and a last of one; 257 x 2

WGRAD3 = [
    (1, 24, 64, 64, 128), (1, 40, 64, 64, 64),      # 12 and 10 rows per slab
    (2, 5, 16, 64, 64), (1, 3, 64, 128, 64),        # odd H, one slab per image
    (1, 1, 32, 64, 128), (1, 2, 16, 64, 64),        # H below the three-row prologue
    (1, 16, 192, 64, 192),                          # three strips with real halo columns, three 64-column chunks
    (1, 48, 32, 192, 128),                          # three input-channel chunks, 24 rows per slab
]

CONV3S_CIN96 = [(2, 8, 32, 96, 64), (1, 8, 16, 96, 128), (3, 16, 32, 96, 128)]      # 27 K-step pairs
CONV3S_ONE_ROW = (3, 4, 32, 64, 64)                 # one patch row: the halo rows above and below are all padding

STEM4 = [(1, 4, 32), (2, 12, 96), (1, 36, 32), (3, 8, 64)]     # (N, Ho, Wo), Ho != Wo; a single tile

# (N, H, W, Cin, Cout, k, stride, pad, dil): the fp32 family (csrc/conv_f32.hip).  Where each lands without a dsnt_out_bounds; with
# one (amax / amax_bn) the K-split cases run on the 32 x 128 tiling.  M = output rows, K = k * k * Cin, a K-step = 32 of K.
CONV_F32 = [
    # ---- the K-split kernel (at most 2048 rows, Cout >= 128, Cin % 8 == 0): eight waves share the chunks of K
    (1, 6, 6, 24, 128, 3, 1, 1, 1),         # chunk width 8 (Cin % 16 != 0), 27 chunks: 3 or 4 per wave; M = 36
    (2, 5, 5, 8, 144, 1, 1, 0, 1),          # width 8, ONE chunk: seven idle waves; Cout % 32 != 0 (out-of-range weight rows); M = 50
    (1, 8, 8, 48, 176, 3, 2, 1, 1),         # width 16, 27 chunks: 3 or 4 per wave; stride 2; ragged Cout; M = 16
    (1, 9, 9, 32, 128, 3, 1, 2, 2),         # width 16, 18 chunks: 2 or 3 per wave; dilation 2; M = 81
    (1, 4, 4, 384, 128, 1, 1, 0, 1),        # width 16, 24 chunks: exactly 3 per wave (the rotation once round); M = 16, half a tile
    (1, 4, 8, 4096, 128, 1, 1, 0, 1),       # 32 chunks per wave; with a prologue the two BatchNorm vectors fill 8192 of the 8448 LDS floats
    (1, 4, 8, 4104, 128, 1, 1, 0, 1),       # width 8, 64 or 65 chunks per wave; with a prologue past the Cin limit: 32 x 128, general loader
    (2, 32, 32, 32, 128, 1, 1, 0, 1),       # M = 2048: the last K-split row count; two chunks, six idle waves
    (1, 2049, 1, 32, 128, 1, 1, 0, 1),      # M = 2049: 32 x 128, FAST, ONE K-step (the loader waves' loop never runs), ragged M
    # ---- the tiled kernels
    (2, 9, 9, 32, 96, 3, 1, 1, 1),          # 128 x 128 FAST, 9 K-steps (odd), ragged M (162) and N (96)
    (1, 10, 10, 12, 72, 5, 1, 2, 1),        # 128 x 128 general, 10 K-steps with a tail (K = 300), ragged M (100) and N (72)
    (1, 128, 128, 32, 160, 1, 1, 0, 1),     # 128 x 128 FAST, one K-step, two N tiles (the second masked past column 160), 256 workgroups
    (2, 17, 15, 32, 64, 3, 2, 1, 1),        # 128 x 64 FAST with stride 2, 9 K-steps, odd image sizes, M = 144
    (2, 7, 9, 16, 48, 1, 1, 0, 1),          # 128 x 64 general, one K-step with a tail (K = 16), ragged N (48), M = 126
    (1, 12, 12, 32, 64, 5, 1, 2, 1),        # 128 x 64 general although Cin % 32 == 0: 25 taps x 4 row passes > 64 mask bits; 25 K-steps
    (1, 11, 13, 20, 16, 3, 1, 1, 1),        # 128 x 32 general, 6 K-steps with a tail (K = 180), ragged N (16), M = 143
    (1, 7, 5, 96, 32, 1, 1, 0, 1),          # 128 x 32 FAST, 3 K-steps, a full 32-column tile, M = 35
    (1, 64, 64, 16, 256, 1, 1, 0, 1),       # 32 x 128 general: the score_ launch (16 -> 256 at 64 x 64), one K-step with a tail
    (1, 6, 7, 12, 128, 3, 1, 1, 1),         # 32 x 128 general from Cin % 8 != 0 at few rows (42), 4 K-steps with a tail (K = 108)
    (3, 30, 30, 32, 144, 3, 1, 1, 1),       # 32 x 128 FAST, 9 K-steps, ragged M (2700) and N (144), 170 workgroups (not a multiple of 8)
]

# (N, H, W, Cin, Cout, R, S, stride, pad, dil) — R and S apart: the tiled bf16x6 / fp16x3 kernels of csrc/conv_split6.hip
# (plan_ref.conv_split).  M = output rows, a K-step = 16 of K = R * S * Cin, a chunk = 16 input channels of the halo kernel.  Cases
# at an odd index run with their weight planes 8 elements further apart than the weights are long.
CONV_SPLIT = [
    # ---- the implicit GEMM (anything the halo kernel does not take)
    (1, 3, 5, 16, 4, 1, 1, 1, 0, 1),        # ONE K-step; M = 15; Cout = 4: one float4 column of a 64-wide tile
    (1, 8, 16, 32, 64, 1, 1, 1, 0, 1),      # two K-steps; exactly one full 128 x 64 tile
    (1, 3, 43, 48, 68, 1, 1, 1, 0, 1),      # three K-steps (the odd tail); M = 129: a row tile of ONE row; Cout = 68 on a 128-wide tile
    (2, 7, 9, 16, 132, 3, 3, 1, 1, 1),      # the tap changes every K-step (9); a second N tile of four columns; two images in one tile
    (3, 5, 7, 16, 64, 3, 3, 1, 1, 1),       # three images in one ragged tile (M = 105)
    (1, 9, 11, 32, 192, 1, 3, 1, 1, 1),     # R != S; Ho = 11 > H: the first and last output rows see padding only; three 64-wide tiles
    (1, 12, 10, 16, 8, 4, 4, 2, 1, 1),      # 16 taps (bit 31 of the tap mask) at stride 2; M = 30
    (1, 15, 13, 48, 128, 3, 3, 2, 1, 1),    # stride 2, odd sizes, 27 K-steps, three per tap; 128 columns as two 64-wide tiles
    (1, 11, 14, 32, 96, 3, 2, 2, 2, 2),     # R != S with stride 2 and dilation 2; Cout = 96 on a 128-wide tile
    (1, 4, 8, 528, 72, 1, 1, 1, 0, 1),      # 33 K-steps; the prologue's vectors copied in three trips, the last ragged; LDS above 64 KB
    (2, 64, 64, 16, 128, 1, 1, 1, 0, 1),    # M = 8192: the last row count on 64-wide tiles
    (1, 65, 128, 16, 128, 1, 1, 1, 0, 1),   # M = 8320: the same channels on 128-wide tiles; 65 row tiles (not a multiple of 8)
    # ---- the LDS halo-tile kernel (3x3 / 1 / 1, H % 8 == 0, W % 16 == 0, Cin % 32 == 0): tiles are 8 x 16 patches
    (1, 8, 16, 32, 4, 3, 3, 1, 1, 1),       # one tile, every halo edge padding; TN = 1; one float4 column; two chunks
    (2, 8, 48, 64, 36, 3, 3, 1, 1, 1),      # TN = 1, ragged Cout; one tile row of three tiles, two images
    (1, 24, 16, 96, 64, 3, 3, 1, 1, 1),     # TN = 1, a full tile; three tile rows in one column; six chunks
    (1, 16, 32, 160, 132, 3, 3, 1, 1, 1),   # TN = 2; ten chunks; 2 x 2 tiles; a second N tile of four columns
    (3, 8, 16, 32, 128, 3, 3, 1, 1, 1),     # TN = 2, full; three one-tile images
]
