"""CPU: where a Winograd layer that does not fit its scratch is cut into groups of tiles (gvx_api.hip, winograd_group_tiles): every
group but the last is a whole number of rounds of the batched products' 128 x 128 tiles, read off gvx_debug_gemm_plan_batched - only
the last group's products end in a remainder launch.  Host arithmetic: no device is touched."""
import ctypes as C

from genvox_amd import _lib


def _fns():
    lib = _lib.load()
    cut = lib.gvx_debug_winograd_group_tiles
    cut.restype, cut.argtypes = C.c_long, [C.c_long, C.c_long, C.c_int]
    plan = lib.gvx_debug_gemm_plan_batched
    plan.restype, plan.argtypes = C.c_int, [C.c_int] * 4 + [C.POINTER(C.c_int)] * 2

    def batched(M, N, K, slices):
        tile, rows_big = C.c_int(), C.c_int()
        assert plan(M, N, K, slices, C.byref(tile), C.byref(rows_big)) == 0
        return tile.value, rows_big.value

    return cut, batched


def _whole_rounds(batched, rows, C_, slices=8):
    """`rows` rows of the batched plan are whole rounds: big tiles, no remainder launch, a multiple of 256 tiles of 128 x 128."""
    tile, rows_big = batched(rows, C_, C_, slices)
    return tile == 4212 and rows_big == 0 and rows % 128 == 0 and (rows // 128) * ((C_ + 127) // 128) * slices % 256 == 0


def test_the_cut_is_a_multiple_of_a_round():
    cut, batched = _fns()
    # 32 x 800 frames, 512 channels: 6400 tiles, 4096 fit the 128 MiB group budget.  The equal cut (3200 + 3200) has a remainder
    # launch in both groups (plan (3200, 512, 512, 8): 3072 rows of big tiles); cut on rounds, 3072 + 3328, only in the last one.
    assert batched(6400, 512, 512, 8) == (4212, 6144) and batched(3200, 512, 512, 8) == (4212, 3072)
    per = cut(6400, 4096, 512)
    assert per == 3072 and _whole_rounds(batched, per, 512) and 6400 - per <= 4096
    # 3200 tiles where 2048 fit: rounding the equal cut (1600) down would leave 2176 for the last group, so it is rounded up
    per = cut(3200, 2048, 512)
    assert per == 2048 and _whole_rounds(batched, per, 512)
    # every cut is whole rounds where the equal cut has the big-tile plan (1536 rows and more), and no group exceeds the scratch
    for total in (3200, 6400, 12800, 51200):
        for fit in (2048, 3000, 4096):
            if fit >= total:
                continue
            per = cut(total, fit, 512)
            assert 1 <= per <= fit and _whole_rounds(batched, per, 512), (total, fit, per)


def test_the_cut_degenerates():
    cut, batched = _fns()
    for total in (1, 7, 1000, 4096):
        assert cut(total, 4096, 512) == total                 # everything fits: one group
    assert cut(1000, 600, 512) == 500                         # a round (1024 tiles) does not fit the scratch: the equal cut
    assert cut(66, 5, 512) == 5 and cut(66, 1, 512) == 1      # the debug limits of the tests: few tiles, small-tile plans
    assert cut(400, 300, 64) == 200                           # narrow layers: not the big-tile plan, nothing to round to
    assert cut(0, 5, 512) == -1 and cut(5, 0, 512) == -1
