"""The exact-integer CutlassMLP shapes — TEST INFRASTRUCTURE ONLY (shared by test_cutlass_cases.py, which asserts their
domain on the CPU, and test_gpu_cutlass_exact.py, which runs them on the device).

n_in, n_out, W, N, n, batch capacity, seed (tests/int_net.py builds the network). What each shape reaches in ffmlp.hip's
wide kernels (k_ff_layer_wide: 128-row output tiles x 256 samples per block, k in chunks of 64; k_ff_wgrad_wide: 128 x 128
tiles x ceil(n / 256) <= 32 sample slices of per = ceil(n / slices) samples, in chunks of 64):
* 24,3,48,2 n 256: a width only CutlassMLP accepts, still on the kernels of the narrow widths;
* 8,5,144,2 n 128: the smallest wide width: a second row tile of 16 rows (one of its four MFMA tiles), K = 144 = two
  chunks and one k-step, half of a block's sample groups empty;
* 20,3,256,2 n 1152 then 2176 on one module of capacity 4096: 5 slices of 231 and 9 of 242 samples (3 chunks + a ragged
  one, unaligned slice starts), the second call's partial rows beside the first's, n below the capacity;
* 40,4,272,3 n 384: a width that is no multiple of 32 (the third row tile has 16 rows), K = 48 in layer 0, three hidden
  layers, 3 x 3 weight-gradient tiles with a 16-wide edge;
* 128,128,512,1 n 256: O = 512 and K = 512 on every side, 128 inputs and outputs without a padding column;
* 3,16,512,3 n 2176 of 4096: 512 x 512 weight gradients (16 tiles) over 9 ragged slices;
* 3,16,144,1 n 131200: k_ff_layer_wide's second stride trip (512 blocks x 256 samples, then 128 more) and all 32 slices."""
SHAPES = [
    (24, 3, 48, 2, 256, 256, 0),
    (8, 5, 144, 2, 128, 128, 0),
    (20, 3, 256, 2, 1152, 4096, 0),
    (20, 3, 256, 2, 2176, 4096, 0),
    (40, 4, 272, 3, 384, 384, 0),
    (128, 128, 512, 1, 256, 256, 0),
    (3, 16, 512, 3, 2176, 4096, 0),
    (3, 16, 144, 1, 131200, 131200, 0),
]
