"""The shapes at which the generator backwards' weight and bias gradients run several pieces across several rows, shared by the GPU
tests that run them (test_melgan_backward_gpu.py, test_hifigan_backward_gpu.py) and by the CPU test that asserts, from the lengths
alone, that every shape still contains the situations it was chosen for (test_backward_piece_layouts_cpu.py).  It also restates both
piece layouts in plain Python.  It imports nothing from genvox_amd.

Both backwards cut the positions a gradient reduces over into pieces of PIECE = 512 (MGB_PIECE, HGB_PIECE); a layer at `mul` positions
per frame has Lmax = T * mul positions per row, of which row b's first T_b * mul are live.
    MelGAN    lays the rows end to end and cuts that line of B * Lmax positions: position g is row g // Lmax, position g % Lmax.  The
              matrix kernel loads 32 consecutive positions of the line at a time (a k-tile), each thread deciding its own row.
    HiFi-GAN  cuts every row on its own into ppr = ceil(Lmax / 512) pieces: piece p is row p // ppr and starts at (p % ppr) * 512."""

PIECE = 512
KTILE = 32

# (config, B, T, lens) - lens None: every row has T frames
MELGAN_CASES = [("NARROW", 3, 350, None), ("SHALLOW", 3, 350, None),
                ("NARROW", 3, 1030, (300, 4, 301)), ("SHALLOW", 3, 1030, (300, 4, 301)),
                ("DEFAULT", 4, 32, None), ("DEFAULT", 4, 33, (33, 5, 32, 17))]
MELGAN_LINEAR_CASE = ("DEFAULT_LINEAR", 4, 32, None)   # slope 1: plain autograd, no tape reading
HIFIGAN_CASES = [("NARROW", 2, 513, None), ("TWO", 2, 513, None),
                 ("NARROW", 3, 1030, (513, 1, 1030)), ("TWO", 3, 1030, (513, 1, 1030)),
                 ("MID", 3, 300, (300, 1, 129)), ("V1", 3, 17, (17, 1, 16))]


def layer_muls(rates):
    """Positions per frame of the layers whose gradients are reduced: 1 (the first convolution and the first transposed convolution's
    weight), then every stage's (its transposed convolution's bias, its residual layers, the next stage's weight; the last: the output
    convolution)."""
    muls, mul = [1], 1
    for r in rates:
        mul *= r
        muls.append(mul)
    return muls


def melgan_pieces(B, T, lens, mul):
    """One dict per piece of the line of B * T * mul positions: first, end (the piece's span of the line), rows (every row it
    touches, in order), live (how many of its positions lie inside their row's length), starts_inside_row (its first position is not a
    row's first), starts_at_row (it is, for a row other than row 0)."""
    Lmax, lens = T * mul, lens or (T,) * B
    total, out = B * Lmax, []
    for first in range(0, total, PIECE):
        end = min(first + PIECE, total)
        rows = list(range(first // Lmax, (end - 1) // Lmax + 1))
        live = sum(max(0, min(end, b * Lmax + lens[b] * mul) - max(first, b * Lmax)) for b in rows)
        out.append(dict(first=first, end=end, rows=rows, live=live, starts_inside_row=first % Lmax != 0,
                        starts_at_row=first % Lmax == 0 and first > 0))
    return out


def melgan_straddling_ktiles(B, T, lens, mul):
    """The first positions of the k-tiles (32 positions of the line, from a piece's start) that hold live positions of two rows."""
    Lmax, lens = T * mul, lens or (T,) * B
    total, out = B * Lmax, []
    for g0 in range(0, total, KTILE):   # PIECE is a multiple of KTILE: the tiles of all pieces together tile the line
        live_rows = {g // Lmax for g in range(g0, min(g0 + KTILE, total)) if g % Lmax < lens[g // Lmax] * mul}
        if len(live_rows) > 1:
            out.append(g0)
    return out


def hifigan_ppr(T, mul):
    return (T * mul + PIECE - 1) // PIECE


def hifigan_pieces(B, T, lens, mul):
    """One dict per piece, B * ppr of them: row, q_base (its first position in the row), live (how many of its positions lie inside
    the row's length; 0: the piece lies wholly behind it)."""
    ppr, lens = hifigan_ppr(T, mul), lens or (T,) * B
    return [dict(row=p // ppr, q_base=(p % ppr) * PIECE, live=max(0, min(PIECE, lens[p // ppr] * mul - (p % ppr) * PIECE))) for p in range(B * ppr)]
