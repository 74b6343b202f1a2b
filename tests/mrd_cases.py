"""The row lengths of the multi-resolution discriminator's GPU tests, and the constants of csrc/mrd.hip they were chosen for.  Shared by
tests/test_mrd_cpu.py (which checks that the lengths hold what is said here, without a GPU) and tests/test_mrd_gpu.py.

A position is a cell (frame, bin) of a map, numbered frame * F + bin; every F is 2^k + 1, so tiles never line up with frames.  The
VALU kernels (the first layer, the score) and the matrix kernels of a layer with c_out % 64 == 0 (HANN) take TILE = 64 positions per
workgroup, the matrix kernels otherwise (DEFAULT, 32 channels) TILE_NARROW = 128.  A weight gradient is summed in pieces of
PIECE_FRAMES = 16 output frames of one row.

LENGTHS[name] holds, for each config:
  - its min_samples (905 for DEFAULT, where the frames reach width 1 behind the strides; 225 for HANN), and 905 in both;
  - for every resolution and every strided layer (inputs: maps 0, 1, 2) an odd and an even input width;
  - CROSS[name]: the n at which the first map of the resolution with most frames has k * TILE + 1 positions (65 frames of 257 bins);
  - PIECES[name]: four n at which some first map has exactly PIECE_FRAMES and PIECE_FRAMES + 1 frames (the VALU weight gradient of
    the first layer: exactly one piece, and one piece plus one frame) and some second map has (the matrix weight gradient of layer 1);
and stays below about 4000 samples."""
from tests import mrd_ref64 as MR

TILE, TILE_NARROW, PIECE_FRAMES = 64, 128, 16
CFGS = dict(DEFAULT=MR.DEFAULT, HANN=MR.HANN)
LENGTHS = dict(DEFAULT=(905, 1550, 1650, 1920, 2040, 3250), HANN=(225, 905, 1024, 1088, 1984, 2112, 4160))
CROSS = dict(DEFAULT=3250, HANN=4160)
PIECES = dict(DEFAULT=(1920, 2040, 1550, 1650), HANN=(1024, 1088, 1984, 2112))   # first map 16, 17 frames; second map 16, 17 frames
