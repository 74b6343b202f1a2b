"""CPU: the host halves of the batched text-to-waveform path - how Synthesizer.tts_batch turns sentences into padded decoder
calls (plan_tts_batches) and how AudioProcessor refuses bad per-row frame counts before anything reaches a GPU."""
import pytest
import torch

from genvox_amd.audio import AudioProcessor
from genvox_amd.configs import AudioConfig
from genvox_amd.dist import plan_shards
from genvox_amd.synthesizer import Synthesizer, plan_tts_batches


def test_plan_pads_and_keeps_lengths():
    sents = [[5, 6, 7], [1], [2, 3, 4, 8, 9], [4, 4]]
    calls = plan_tts_batches(sents, batch_size=32)
    assert len(calls) == 1
    idx, tokens, lens = calls[0]
    assert idx == [2, 0, 3, 1]                                   # longest first
    assert tokens.dtype == torch.int32 and lens.dtype == torch.int32
    assert tokens.tolist() == [[2, 3, 4, 8, 9], [5, 6, 7, 0, 0], [4, 4, 0, 0, 0], [1, 0, 0, 0, 0]]
    assert lens.tolist() == [5, 3, 2, 1]


def test_plan_groups_by_length_and_covers_every_sentence_once():
    g = torch.Generator().manual_seed(0)
    n_tok = torch.randint(1, 60, (23,), generator=g).tolist()
    sents = [list(range(1, n + 1)) for n in n_tok]
    calls = plan_tts_batches(sents, batch_size=5)
    assert [len(c[0]) for c in calls] == [5, 5, 5, 5, 3]
    seen = [i for c in calls for i in c[0]]
    assert sorted(seen) == list(range(23))
    assert seen == plan_shards(n_tok, 1)[0]                      # the order dist.plan_shards deals in (ties in input order)
    longest = [int(c[2][0]) for c in calls]
    assert longest == sorted(longest, reverse=True)
    for idx, tokens, lens in calls:
        assert tokens.shape == (len(idx), int(lens.max())) and int(lens[0]) == int(lens.max())
        assert lens.tolist() == sorted(lens.tolist(), reverse=True)
        for r, i in enumerate(idx):
            assert tokens[r, :lens[r]].tolist() == sents[i] and not tokens[r, lens[r]:].any()
    # order restored by writing call results back through the indices
    back = [None] * 23
    for idx, tokens, lens in calls:
        for r, i in enumerate(idx):
            back[i] = tokens[r, :lens[r]].tolist()
    assert back == sents


def test_plan_edge_cases():
    assert plan_tts_batches([], batch_size=4) == []
    one = plan_tts_batches([[3, 1, 2]], batch_size=4)
    assert len(one) == 1 and one[0][0] == [0] and one[0][1].tolist() == [[3, 1, 2]] and one[0][2].tolist() == [3]
    assert [c[0] for c in plan_tts_batches([[1], [2, 2], [3, 3, 3]], batch_size=1)] == [[2], [1], [0]]
    with pytest.raises(ValueError, match="sentence 2"):
        plan_tts_batches([[1], [2], [], [3]], batch_size=4)
    with pytest.raises(ValueError):
        plan_tts_batches([[1]], batch_size=0)
    assert callable(getattr(Synthesizer, "tts_batch"))


def test_frame_lengths_are_validated_on_the_host():
    """device='cpu': a call that got past the validation would raise RuntimeError (there is no CPU vocoder), so a ValueError
    shows that the lengths were refused first."""
    ap = AudioProcessor(AudioConfig(filter_length=1024, hop_length=256), device="cpu")
    mel = torch.zeros(3, 80, 12)
    for bad in ([12, 0, 3], [12, 13, 3], [12, -1, 3], [12, 3], [12, 3, 3, 3]):
        with pytest.raises(ValueError):
            ap.convert_mel2wav_batch(mel, mel_lengths=bad)
    with pytest.raises(ValueError):
        ap.convert_mel2wav_batch(mel, mel_lengths=torch.tensor([12, 40, 3]))
    with pytest.raises(RuntimeError):
        ap.convert_mel2wav_batch(mel, mel_lengths=[12, 1, 3])     # valid lengths: stopped only by the missing GPU
    assert ap.row_samples([12, 1, 3]) == [1024 + 11 * 256 - 1000, 24, 1024 + 2 * 256 - 1000]
    assert ap.row_samples([2], trimmed=False) == [1280]
    short = AudioProcessor(AudioConfig(filter_length=512, hop_length=128), device="cpu")
    with pytest.raises(ValueError, match="too short"):
        short.convert_mel2wav_batch(mel, mel_lengths=[12, 4, 5])  # 896 samples cannot lose 500 at both ends
