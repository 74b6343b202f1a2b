"""GPU: the encoder's three 512 -> 512, 5-tap convolutions as Winograd F(4,5) (gvx_api.hip encoder_impl, winograd_conv.hip with the
ReLU output transform), through gvx_encoder_forward and inside gvx_tacotron2_forward.

What gates is tests/test_forward_loops_gpu.py's own yardstick: per position, max |got - float64| <= TOL["enc_whole"] x the
position's largest |float64| (error / bound <= 1), reference tests/forward_ref.py::whole_encoder.  On top of it the tighter
WINOGRAD_RATIO_LIMIT: four times the worst Winograd error / bound the first run of this file on an MI355X measured over its
shapes and both weight sets.  Measured: 1.691e-01 of the bound (B = 3, L = 1, plain weights), against 1.008e-01 for the direct form
(mode 0) over the same shapes (B = 2, L = 131, peaky weights); shape by shape the Winograd figure is 1.1 to 1.9 times the direct
one, and most of both is the fp32 recurrence behind the convolutions.  The factor 4 leaves room for other seeds.

The path is chosen by (cin, cout, k) and the handle's mode alone, tiles of four positions start at position 0 of each sequence, and
V / M live in workspace regions that are dead while the convolutions run: neither the batch a row runs in, nor where a group of
tiles ends, nor what the workspace held, nor the Prenet products that run beside the encoder in the fused forward may change a bit."""
import ctypes as C

import pytest
import torch

from genvox_amd import _lib, weights as gw
from tests import forward_ref as fr
from tests import test_forward_loops_gpu as F
from tests.helpers import bptt_lengths, fwd_configs
from tests.test_bptt_gpu import _Out

pytestmark = pytest.mark.gpu

MEASURED_WORST_RATIO = 1.691e-01    # Winograd error / bound, the worst of the first GPU run (module docstring)
MEASURED_WORST_DIRECT = 1.008e-01   # the direct form's, same shapes (not asserted: what the Winograd figure is read against)
WINOGRAD_RATIO_LIMIT = 4.0 * MEASURED_WORST_RATIO

# below one tile, at and around tile edges, a last tile that sticks out into the next sequence's rows, more tiles than one small group
SHAPES = [(3, 1), (3, 2), (3, 3), (3, 4), (3, 5), (3, 7), (3, 8), (3, 9), (2, 131)]
CLEAR = 12804   # GVX_WORKSPACE_CLEAR_BYTES: the status words up to and including the hand-off time-out word

_REFS, _BLOBS = {}, {}


def _weights(cfgs, wset):
    """(state dict, packed blob on the device) of the default layer sizes and a weight set of test_forward_loops_gpu."""
    from genvox_amd.tacotron2 import Tacotron2

    if wset[0] not in _BLOBS:
        sd = gw.generate_state_dict(*cfgs, seed=wset[1], peaky_attention=wset[2])
        m = Tacotron2(*cfgs)
        m.load_state_dict(sd)
        _BLOBS[wset[0]] = (sd, m.pack_weights_host().cuda())
    return _BLOBS[wset[0]]


@pytest.fixture(scope="module")
def lib():
    lib = _lib.load()
    lib.gvx_debug_set_winograd_group.restype, lib.gvx_debug_set_winograd_group.argtypes = C.c_int, [C.c_void_p, C.c_int]
    yield lib
    for h in _OWN:
        lib.gvx_model_destroy(h)
    _OWN.clear()
    _REFS.clear()
    _BLOBS.clear()


_OWN = []


def _own_handle(lib, cfgs, wset, mode):
    """A handle of this module's own (the modes and group limits set here must not reach the handles other modules share)."""
    from genvox_amd.tacotron2 import dims_from_configs
    from tests.helpers import create_handle

    h = create_handle(lib, dims_from_configs(*cfgs))
    _OWN.append(h)
    assert lib.gvx_model_bind_blob(h, _weights(cfgs, wset)[1].data_ptr()) == 0, lib.gvx_last_error()
    assert lib.gvx_model_set_winograd(h, mode) == 0
    return h


@pytest.fixture(scope="module")
def handles(lib):
    cfgs = fwd_configs("def")
    return {(w[0], mode): _own_handle(lib, cfgs, w, mode) for w in F.WEIGHT_SETS for mode in (0, 1)}


def _case(B, L, salt):
    cfgs = fwd_configs("def")
    g = F._gen("wino_enc_%dx%d" % (B, L), salt)
    lengths = bptt_lengths("ragged", B, L)
    return torch.randint(0, cfgs[2].n_tokens, (B, L), generator=g), lengths


def _encode(lib, h, tokens, lengths, fill=0x00):
    """gvx_encoder_forward on exactly gvx_workspace_bytes_autoregressive(B, L, 1) bytes, filled with `fill` behind the status words."""
    B, L = tokens.shape
    E = fwd_configs("def")[0].encoder_embedding_dim
    n = lib.gvx_workspace_bytes_autoregressive(h, B, L, 1)
    ws = torch.full((n + 256,), fill, dtype=torch.uint8, device="cuda")
    ws[:CLEAR] = 0
    ws[n:] = 0xA5
    out = _Out((B, L, E), junk=True)
    tok, ln = tokens.cuda(), torch.tensor(lengths, dtype=torch.int32).cuda()
    rc = lib.gvx_encoder_forward(h, tok.data_ptr(), ln.data_ptr(), B, L, out.t.data_ptr(), ws.data_ptr(), n, F._stream())
    torch.cuda.synchronize()
    assert rc == 0 and out.border_intact(), (rc, lib.gvx_last_error())
    assert bool((ws[n:] == 0xA5).all()), "gvx_encoder_forward wrote behind its workspace"
    return out.t.clone()


def _ratio(got, want):
    """The worst error / bound of test_forward_loops_gpu._compare, per position (got / want [B, L, E])."""
    got, want = got.double().cpu().transpose(0, 1), want.double().transpose(0, 1)
    worst = 0.0
    for t in range(got.shape[0]):
        scale = float(want[t].abs().max())
        if scale > 0.0:
            worst = max(worst, float((got[t] - want[t]).abs().max()) / (F.TOL["enc_whole"] * scale))
    return worst


@pytest.mark.parametrize("B,L", SHAPES)
def test_against_float64_both_modes(lib, handles, B, L):
    """Modes 0 and 1, both weight sets, on a workspace full of 0xFF: _compare's bound, zeros behind each row's length, and the
    tighter limit on the Winograd form."""
    cfgs = fwd_configs("def")
    for wset in F.WEIGHT_SETS:
        tokens, lengths = _case(B, L, wset[1])
        key = (B, L, wset[0])
        if key not in _REFS:
            _REFS[key] = fr.whole_encoder(fr.to_f64(_weights(cfgs, wset)[0]), tokens, lengths)["memory"]
        want = _REFS[key]
        pad = fr.pad_mask(lengths, L).cuda()
        worst = {}
        for mode in (0, 1):
            h = handles[wset[0], mode]
            assert lib.gvx_debug_conv_plan(h, 512, 512, 5) == mode
            out = _encode(lib, h, tokens, lengths, 0xFF)
            worst[mode] = _ratio(out, want)
            F._compare("enc_whole", out.transpose(0, 1), want.transpose(0, 1), f"wino_enc_{B}x{L}/{wset[0]}/mode{mode}")
            assert bool((out[pad] == 0).all()), (B, L, wset[0], mode)
        print(f"winograd encoder B={B} L={L} {wset[0]}: error / bound direct {worst[0]:.3e} winograd {worst[1]:.3e}")
        assert worst[1] <= WINOGRAD_RATIO_LIMIT, (B, L, wset[0], worst)


def test_the_path_ran_and_the_plan_answers_as_before(lib, handles):
    """The two forms round differently: equal outputs would mean the Winograd path did not run.  gvx_debug_conv_plan is unchanged."""
    tokens, lengths = _case(3, 9, 0)
    a, b = _encode(lib, handles["plain", 0], tokens, lengths), _encode(lib, handles["plain", 1], tokens, lengths)
    assert not torch.equal(a, b)
    plan = lambda mode, *shape: lib.gvx_debug_conv_plan(handles["plain", mode], *shape)
    assert plan(1, 512, 512, 5) == 1 and plan(1, 256, 256, 5) == 1 and plan(1, 64, 64, 5) == 0 and plan(1, 512, 512, 3) == 0 and plan(1, 80, 512, 5) == 0
    assert plan(0, 512, 512, 5) == 0 and plan(0, 64, 64, 5) == 0


def test_group_boundaries_change_no_bit(lib, handles):
    """Groups of 1 and 5 tiles and of one sequence's tiles (L = 131 is 33 tiles) give the bits of one group."""
    h = handles["peaky", 1]
    tokens, lengths = _case(2, 131, 1)
    one_group = _encode(lib, h, tokens, lengths)
    try:
        for tiles in (1, 5, 33):
            assert lib.gvx_debug_set_winograd_group(h, tiles) == 0
            assert torch.equal(one_group, _encode(lib, h, tokens, lengths)), tiles
    finally:
        assert lib.gvx_debug_set_winograd_group(h, 0) == 0


@pytest.mark.parametrize("L", [5, 9])
def test_a_row_does_not_depend_on_its_batch(lib, handles, L):
    """Row b of a B = 3 call equals the B = 1 call with that row's tokens, the same padded L and the same length, bit for bit: the
    tile indices differ, the values must not."""
    h = handles["plain", 1]
    tokens, lengths = _case(3, L, 0)
    batch = _encode(lib, h, tokens, lengths)
    for b in range(3):
        alone = _encode(lib, h, tokens[b:b + 1].contiguous(), lengths[b:b + 1])
        assert torch.equal(batch[b], alone[0]), (L, b)


@pytest.mark.parametrize("B,L,T", [(5, 24, 5), (32, 128, 6)])
def test_inside_the_fused_forward(lib, handles, B, L, T):
    """gvx_tacotron2_forward on a workspace full of 0xFF behind the status words: the encoder output in its workspace equals the
    stand-alone gvx_encoder_forward's bit for bit - the Prenet products that run beside the convolutions touch no scratch of theirs."""
    cfgs = fwd_configs("def")
    mc, ac, tc = cfgs
    M, P, E = ac.n_mels, mc.prenet_dim, mc.encoder_embedding_dim
    h = handles["peaky", 1]
    tokens, lengths = _case(B, L, 1)
    alone = _encode(lib, h, tokens, lengths)
    g = F._gen(f"wino_fused_{B}x{L}x{T}", 0)
    mel_in = torch.randn(B, M, T, generator=g).cuda()
    keep = (torch.rand(2, (T + 1) * B, P, generator=g) < 0.5).to(torch.uint8).cuda()
    tok, tl = tokens.cuda(), torch.tensor(lengths, dtype=torch.int32).cuda()
    n = lib.gvx_workspace_bytes(h, B, L, T)
    ws = torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda")
    ws[:CLEAR] = 0
    mel, gate, align = _Out((B, M, T), junk=True), _Out((B, T), junk=True), _Out((B, T, L), junk=True)
    rc = lib.gvx_tacotron2_forward(h, tok.data_ptr(), tl.data_ptr(), B, L, mel_in.data_ptr(), None, T, keep.data_ptr(), mel.t.data_ptr(), None,
                                   gate.t.data_ptr(), align.t.data_ptr(), ws.data_ptr(), n, F._stream())
    torch.cuda.synchronize()
    assert rc == 0, (rc, lib.gvx_last_error())
    memory = _Out((B, L, E), junk=True)
    assert lib.gvx_train_export(h, ws.data_ptr(), n, B, L, T, 4, memory.t.data_ptr(), F._stream()) == 0, lib.gvx_last_error()
    torch.cuda.synchronize()
    assert memory.border_intact() and mel.border_intact() and bool(torch.isfinite(mel.t).all())
    assert torch.equal(memory.t, alone)


# ---- the transformed weights follow the model ---------------------------------------------------------------------------------
def _narrow_configs():
    """Everything small, the encoder 32 channels wide with 5 taps: the smallest width Winograd mode 2 admits."""
    from genvox_amd.configs import AudioConfig, Tacotron2Config, TextConfig
    from tests.helpers import FWD_DIMS

    d = dict(FWD_DIMS["small"]["model"], encoder_kernel_size=5)
    return Tacotron2Config(**d), AudioConfig(filter_length=1024, hop_length=256, n_mels=FWD_DIMS["small"]["n_mels"], log_func="np.log"), TextConfig(n_tokens=40)


def _narrow_model(sd):
    from genvox_amd.tacotron2 import Tacotron2

    m = Tacotron2(*_narrow_configs())
    m.load_state_dict(sd)
    m = m.to("cuda:0")
    m.set_winograd(2)
    assert m.conv_plan(32, 32, 5) == 1
    return m


def _narrow_encode(m, tokens, lengths):
    """gvx_encoder_forward of a Tacotron2 object's own handle and blob."""
    lib = _lib.load()
    m._ensure_packed()
    return _encode_dims(lib, m._handle, tokens, lengths, 32)


def _encode_dims(lib, h, tokens, lengths, E):
    B, L = tokens.shape
    n = lib.gvx_workspace_bytes_autoregressive(h, B, L, 1)
    ws = torch.zeros(n, dtype=torch.uint8, device="cuda")
    out = torch.empty(B, L, E, device="cuda")
    tok, ln = tokens.cuda(), torch.tensor(lengths, dtype=torch.int32).cuda()
    rc = lib.gvx_encoder_forward(h, tok.data_ptr(), ln.data_ptr(), B, L, out.data_ptr(), ws.data_ptr(), n, F._stream())
    torch.cuda.synchronize()
    assert rc == 0, (rc, lib.gvx_last_error())
    return out


def test_transformed_weights_follow_a_new_state_dict():
    """Seed-A weights, a run, seed-B weights into the same model, a run: the bits of a fresh model with seed B; and mode 0 differs."""
    cfgs = _narrow_configs()
    sd_a, sd_b = gw.generate_state_dict(*cfgs, seed=31), gw.generate_state_dict(*cfgs, seed=32)
    tokens, lengths = torch.randint(0, 40, (2, 11), generator=torch.Generator().manual_seed(5)), [11, 6]
    m = _narrow_model(sd_a)
    out_a = _narrow_encode(m, tokens, lengths)
    m.load_state_dict(sd_b)
    out_b = _narrow_encode(m, tokens, lengths)
    fresh = _narrow_model(sd_b)
    assert torch.equal(out_b, _narrow_encode(fresh, tokens, lengths)) and not torch.equal(out_a, out_b)
    fresh.set_winograd(0)
    assert not torch.equal(out_b, _narrow_encode(fresh, tokens, lengths)), "mode 2 did not reach the narrow encoder's Winograd path"


def test_transformed_weights_follow_a_train_step():
    """One tiny train_step re-packs the blob on the device: the encoder in eval mode afterwards gives the bits of a fresh model
    loaded from the stepped state_dict (whose blob the host packs)."""
    from tests import train_ref64 as R
    from tests.helpers import train_step_mel_lengths

    mc, ac, tc = _narrow_configs()
    B, L, T = 3, 6, 7
    m = _narrow_model(gw.generate_state_dict(mc, ac, tc, seed=33))
    tokens, lengths = torch.randint(0, 40, (2, 11), generator=torch.Generator().manual_seed(6)), [11, 6]
    before = _narrow_encode(m, tokens, lengths)
    inp = gw.synthetic_inputs(B, L, T, tc.n_tokens, ac.n_mels, seed=302, token_lengths=bptt_lengths("ragged", B, L), mel_lengths=train_step_mel_lengths(B, T))
    batch = {k: torch.from_numpy(v) for k, v in inp.items()}
    m.train_step(R.gpu_batch(batch, R.draw_masks(mc, ac.n_mels, B, L, T, 402)), m.get_criterion(), m.get_optimizer())
    m.check_status()
    m.eval()
    after = _narrow_encode(m, tokens, lengths)
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    fresh = _narrow_encode(_narrow_model(sd), tokens, lengths)
    assert torch.equal(after, fresh) and not torch.equal(after, before)
