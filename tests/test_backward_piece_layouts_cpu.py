"""CPU: the shapes of the several-rows-times-several-pieces cases of the MelGAN and HiFi-GAN backward tests (tests/backward_piece_cases.py)
contain the situations they were chosen for.  Everything here follows from B, T, the lengths and the up-sampling rates through a plain
Python restatement of the two piece layouts; an edit to a shape that loses a situation fails here, without a GPU.

The last test is about the references alone: at MelGAN's default sizes, 4 x 32 frames, the float32 restatement with its own LeakyReLU
decisions is far from float64 (a near-tie decided the other way changes a gradient by a finite amount), and pinned to float64's
decisions it is not.  That is why gradients of this shape class are compared with a pinned reference, and what lies between the device
and torch's float32 autograd there."""
import pytest
import torch

from tests import backward_piece_cases as PC
from tests import hifigan_ref64 as HR
from tests import melgan_grad_ref64 as MGR
from tests import melgan_ref64 as MR

MELGAN = dict(NARROW=MR.NARROW, SHALLOW=MR.SHALLOW, DEFAULT=MR.DEFAULT, DEFAULT_LINEAR=MR.DEFAULT)
HIFIGAN = dict(NARROW=HR.NARROW, TWO=HR.TWO, MID=HR.MID, V1=HR.V1)


def _mg(name, B, T, lens, mul):
    assert mul in PC.layer_muls(MELGAN[name]["ratios"]), f"{name} has no layer at {mul} positions per frame"
    return PC.melgan_pieces(B, T, lens, mul), PC.melgan_straddling_ktiles(B, T, lens, mul)


def _hg(name, B, T, lens, mul):
    assert mul in PC.layer_muls(HIFIGAN[name]["rates"]), f"{name} has no layer at {mul} positions per frame"
    return PC.hifigan_ppr(T, mul), PC.hifigan_pieces(B, T, lens, mul)


def test_the_restated_layouts_partition_the_live_positions():
    """Every live position of every row lies in exactly one piece, in both layouts, for every case and layer."""
    for table, cfgs, key in ((PC.MELGAN_CASES + [PC.MELGAN_LINEAR_CASE], MELGAN, "ratios"), (PC.HIFIGAN_CASES, HIFIGAN, "rates")):
        for name, B, T, lens in table:
            for mul in PC.layer_muls(cfgs[name][key]):
                want = sum(lens or (T,) * B) * mul
                mg, hg = PC.melgan_pieces(B, T, lens, mul), PC.hifigan_pieces(B, T, lens, mul)
                assert sum(p["live"] for p in mg) == want and sum(p["live"] for p in hg) == want, (name, B, T, lens, mul)
                assert len(mg) == -(-B * T * mul // PC.PIECE) and len(hg) == B * PC.hifigan_ppr(T, mul)
                for b in range(B):   # HiFi-GAN: a row's pieces hold that row's live positions
                    assert sum(p["live"] for p in hg if p["row"] == b) == (lens or (T,) * B)[b] * mul


def test_every_case_has_several_rows_and_several_pieces():
    for name, B, T, lens in PC.MELGAN_CASES + [PC.MELGAN_LINEAR_CASE]:
        assert B > 1 and max(len(PC.melgan_pieces(B, T, lens, mul)) for mul in PC.layer_muls(MELGAN[name]["ratios"])) > 1
        assert lens is None or (len(lens) == B and max(lens) <= T and min(lens) >= 4)   # 4: GVX_MELGAN_MIN_FRAMES
    for name, B, T, lens in PC.HIFIGAN_CASES:
        assert B > 1 and max(PC.hifigan_ppr(T, mul) for mul in PC.layer_muls(HIFIGAN[name]["rates"])) > 1
        assert lens is None or (len(lens) == B and max(lens) <= T and min(lens) >= 1)


@pytest.mark.parametrize("name", ["NARROW", "SHALLOW"])
def test_melgan_3x350(name):
    """mul = 1: rows begin at 350 and 700, inside pieces 0 and 1 and inside a k-tile (350 = 10 x 32 + 30); piece 1 begins inside row 1."""
    assert (name, 3, 350, None) in PC.MELGAN_CASES
    pieces, straddle = _mg(name, 3, 350, None, 1)
    assert [p["rows"] for p in pieces] == [[0, 1], [1, 2], [2]] and [p["live"] for p in pieces] == [512, 512, 26]
    assert pieces[1]["starts_inside_row"] and pieces[2]["starts_inside_row"]
    assert straddle == [320, 672]
    for mul in (4, 8):   # several pieces per row and pieces holding two rows at every layer
        pieces, straddle = _mg(name, 3, 350, None, mul)
        assert len(pieces) == -(-1050 * mul // 512) and sum(len(p["rows"]) == 2 for p in pieces) == 2 and straddle[0] == 350 * mul // 32 * 32


@pytest.mark.parametrize("name", ["NARROW", "SHALLOW"])
def test_melgan_3x1030_ragged(name):
    """mul = 1: 7 pieces; piece 1 lies wholly behind row 0's 300 frames; row 1 begins at 1030, inside piece 2 and inside the k-tile
    1024..1055; row 2 begins at 2060, inside piece 4; the last piece has 18 positions.  mul = 4 and 8: 25 and 49 pieces, several of
    them wholly dead."""
    lens = (300, 4, 301)
    assert (name, 3, 1030, lens) in PC.MELGAN_CASES
    pieces, straddle = _mg(name, 3, 1030, lens, 1)
    assert len(pieces) == 7 and pieces[1]["live"] == 0 and pieces[1]["rows"] == [0]
    assert pieces[2]["rows"] == [0, 1] and pieces[2]["live"] == 4 and pieces[4]["rows"] == [1, 2] and pieces[4]["live"] == 301
    assert pieces[6]["end"] - pieces[6]["first"] == 18 and pieces[6]["live"] == 0
    assert [p["live"] for p in pieces] == [300, 0, 4, 0, 301, 0, 0]
    assert straddle == []   # no k-tile has live positions of two rows: row 0 ends long before 1030 ...
    assert 1024 < 1030 < 1056 and 2048 < 2060 < 2080   # ... but rows 1 and 2 begin inside a k-tile whose first positions belong to the row before
    for mul, count in ((4, 25), (8, 49)):
        pieces, _ = _mg(name, 3, 1030, lens, mul)
        assert len(pieces) == count and sum(p["live"] == 0 for p in pieces) >= 5
        assert any(0 < p["live"] < 512 and len(p["rows"]) == 2 for p in pieces)   # a piece that ends a dead stretch and begins a row


@pytest.mark.parametrize("name", ["DEFAULT", "DEFAULT_LINEAR"])
def test_melgan_default_4x32(name):
    """The training benchmark's shape class.  mul = 1: one piece holding all four rows; mul = 8: every piece is exactly two rows, so
    piece 1 begins at row 2's first position; mul = 64: four pieces per row."""
    assert (name, 4, 32, None) in PC.MELGAN_CASES + [PC.MELGAN_LINEAR_CASE]
    pieces, straddle = _mg(name, 4, 32, None, 1)
    assert len(pieces) == 1 and pieces[0]["rows"] == [0, 1, 2, 3] and pieces[0]["live"] == 128 and straddle == []
    pieces, _ = _mg(name, 4, 32, None, 8)
    assert [p["rows"] for p in pieces] == [[0, 1], [2, 3]] and pieces[1]["starts_at_row"]
    pieces, _ = _mg(name, 4, 32, None, 64)
    assert len(pieces) == 16 and all(p["rows"] == [i // 4] for i, p in enumerate(pieces)) and sum(p["starts_inside_row"] for p in pieces) == 12
    assert len(_mg(name, 4, 32, None, 128)[0]) == 32 and len(_mg(name, 4, 32, None, 256)[0]) == 64


def test_melgan_default_4x33_ragged():
    """Lmax = 33 and 264 at mul = 1 and 8 is no multiple of 32, so k-tiles straddle rows at the widest layers (512 and 256
    channels); row 1 (5 frames) leaves whole pieces dead from mul = 64 on."""
    name, lens = "DEFAULT", (33, 5, 32, 17)
    assert (name, 4, 33, lens) in PC.MELGAN_CASES
    pieces, straddle = _mg(name, 4, 33, lens, 1)
    # 32..63 holds row 0's last position and row 1's five, 96..127 row 2's last two and row 3's first; 64..95 begins in row 1, behind its length
    assert len(pieces) == 1 and pieces[0]["live"] == 87 and straddle == [32, 96]
    pieces, straddle = _mg(name, 4, 33, lens, 8)
    assert len(pieces) == 3 and straddle == [256, 768] and pieces[1]["rows"] == [1, 2, 3] and pieces[1]["starts_inside_row"]
    for mul in (64, 128, 256):
        pieces, straddle = _mg(name, 4, 33, lens, mul)
        dead_in_row_1 = [p for p in pieces if p["rows"] == [1] and p["live"] == 0]
        assert len(dead_in_row_1) >= 3, mul
        assert any(p["starts_inside_row"] and len(p["rows"]) == 2 and p["live"] > 0 for p in pieces)


@pytest.mark.parametrize("name", ["NARROW", "TWO"])
def test_hifigan_2x513(name):
    """ppr = 2 at mul = 1 with both rows full: pieces 1 and 3 hold one position, and piece 2 is row 1's first."""
    assert (name, 2, 513, None) in PC.HIFIGAN_CASES
    ppr, pieces = _hg(name, 2, 513, None, 1)
    assert ppr == 2 and [(p["row"], p["q_base"], p["live"]) for p in pieces] == [(0, 0, 512), (0, 512, 1), (1, 0, 512), (1, 512, 1)]
    ppr, pieces = _hg(name, 2, 513, None, 4)
    assert ppr == 5 and [p["live"] for p in pieces] == [512, 512, 512, 512, 4] * 2


@pytest.mark.parametrize("name", ["NARROW", "TWO"])
def test_hifigan_3x1030_ragged(name):
    """ppr = 3 at mul = 1: row 0 is full / one position / behind the row, row 1 one position / dead / dead, row 2 full / full / a
    tail of 6.  ppr = 9 at mul = 4."""
    lens = (513, 1, 1030)
    assert (name, 3, 1030, lens) in PC.HIFIGAN_CASES
    ppr, pieces = _hg(name, 3, 1030, lens, 1)
    assert ppr == 3 and [p["live"] for p in pieces] == [512, 1, 0, 1, 0, 0, 512, 512, 6]
    assert [p["row"] for p in pieces] == [0, 0, 0, 1, 1, 1, 2, 2, 2]
    ppr, pieces = _hg(name, 3, 1030, lens, 4)
    assert ppr == 9 and [p["live"] for p in pieces] == [512] * 4 + [4] + [0] * 4 + [4] + [0] * 8 + [512] * 8 + [24]
    last = PC.layer_muls(HIFIGAN[name]["rates"])[-1]
    assert _hg(name, 3, 1030, lens, last)[0] == -(-1030 * last // 512) > 9


def test_hifigan_mid_3x300_ragged():
    """The matrix kernel everywhere.  ppr = 3 at mul = 4, where row 2 has 516 positions: a full piece, a 4-position piece, a dead one;
    ppr = 5 at mul = 8."""
    name, lens = "MID", (300, 1, 129)
    assert (name, 3, 300, lens) in PC.HIFIGAN_CASES
    assert _hg(name, 3, 300, lens, 1)[0] == 1
    ppr, pieces = _hg(name, 3, 300, lens, 4)
    assert ppr == 3 and [p["live"] for p in pieces] == [512, 512, 176, 4, 0, 0, 512, 4, 0]
    ppr, pieces = _hg(name, 3, 300, lens, 8)
    assert ppr == 5 and [p["live"] for p in pieces] == [512] * 4 + [352] + [8] + [0] * 4 + [512, 512, 8, 0, 0]


def test_hifigan_v1_3x17_ragged():
    """The published widths.  ppr = 3, 5, 9 at mul = 64, 128, 256; at mul = 64 row 2's 1024 positions fill exactly two pieces and its
    third is dead."""
    name, lens = "V1", (17, 1, 16)
    assert (name, 3, 17, lens) in PC.HIFIGAN_CASES
    assert [_hg(name, 3, 17, lens, mul)[0] for mul in (1, 8, 64, 128, 256)] == [1, 1, 3, 5, 9]
    _, pieces = _hg(name, 3, 17, lens, 64)
    assert [p["live"] for p in pieces] == [512, 512, 64, 64, 0, 0, 512, 512, 0]
    _, pieces = _hg(name, 3, 17, lens, 256)
    assert [p["live"] for p in pieces if p["row"] == 1] == [256] + [0] * 8 and [p["live"] for p in pieces if p["row"] == 2] == [512] * 8 + [0]


def test_melgan_default_4x32_float32_gap_is_sign_decisions():
    """The references alone, at the case test_melgan_backward_gpu.py runs: with its own LeakyReLU decisions the float32 restatement is
    above 1e-3 of a tensor's scale from float64 in at least one gradient tensor (measured: 6.0e-3 and 1.3e-2 on two hosts, whose
    float32 convolutions add in different orders, with 700 and 718 near-ties in the float64 tape); pinned to float64's decisions
    every tensor is below 1e-4 (measured: 4.8e-6 on both)."""
    name, B, T, _ = PC.MELGAN_CASES[4]
    assert (name, B, T) == ("DEFAULT", 4, 32)
    cfg = MELGAN[name]
    sd, mel = MR.random_state(cfg, seed=11), MR.random_mel(cfg, B, T, 1)
    G = torch.randn(B, T * MR.hop(cfg), generator=torch.Generator().manual_seed(1000 * B + T), dtype=torch.float64)
    free = MGR.reference(sd, mel, None, cfg, G)
    pinned = MGR.reference(sd, mel, None, cfg, G, MGR.masks_from_tape(free["tape"], cfg["slope"]))

    def worst(ref):
        return max(ref["grad_err"][k] / g.abs().max().item() for k, g in ref["grads"].items())

    print(f"{MGR.near_ties(free)} near-ties; float32 restatement from float64, of a tensor's scale: {worst(free):.3e} with its own decisions, "
          f"{worst(pinned):.3e} pinned to float64's")
    assert MGR.near_ties(free) > 0
    assert worst(free) > 1e-3
    assert worst(pinned) < 1e-4
    for a, b in zip(free["tape"], pinned["tape"]):   # pinning to float64's own decisions changes nothing in float64
        assert torch.equal(a, b)
