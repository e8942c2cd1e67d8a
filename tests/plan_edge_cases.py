"""The cases of tests/test_plan_edges_gpu.py, (N, H, W, Cin, Cout) unless said otherwise: geometries the plans of the fp16x3
streaming kernels accept and the hourglass's own shapes never produce.  What each is for — on 256 CUs — is asserted by
tests/test_plan_edges_cpu.py."""

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
