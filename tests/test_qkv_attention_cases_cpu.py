"""The inputs of the fused QKV + attention tests (_qkv_attention_cases.py) have the properties the GPU tests rely on: the token
counts sit on the edges of qkv_attention.hip, the three stress inputs force the rescale branch the way they claim to - replayed
under the kernel's own rule on fp64 scores - and every forward row keeps |logit| <= 16 with an fp32 oracle within 5e-5 of its fp64
evaluation.  Checks the inputs, not the kernel: nothing here needs a GPU (the kernel: test_hip_qkv_attention.py)."""
import pytest
import torch

import _qkv_attention_cases as C

B = 2


def test_token_counts_sit_on_the_kernels_edges():
    assert len(set(C.COUNTS)) == len(C.COUNTS) and min(C.COUNTS) >= 1 and max(C.COUNTS) <= C.MAX_TOKENS
    two = lambda wave, n: wave * 32 + 16 < n  # noqa: E731  (the kernel's `two_tiles`)
    for wave in (0, 1, 5):  # the switch from one to two tiles, on both sides
        assert 32 * wave + 16 in C.COUNTS and not two(wave, 32 * wave + 16)
        assert 32 * wave + 17 in C.COUNTS and two(wave, 32 * wave + 17)
    for wave in (1, 2, 3, 4, 5, 6):  # wave `wave` without a query at N = 32 wave, with one query (and a key step more) at + 1
        assert 32 * wave in C.COUNTS and (32 * wave + 31) >> 5 == wave
        assert 32 * wave + 1 in C.COUNTS or wave in (2, 6)  # 65 and 193 are cases of the parity test itself
    assert {(n + 31) >> 5 for n in C.COUNTS} == {1, 2, 3, 4, 5, 6, 7}  # every number of key steps
    rem = {n % 32 for n in C.COUNTS}
    assert {15, 16, 17} <= rem  # last 16-key tile of the last step: one key masked in the first tile / wholly masked / one valid key
    assert {0, 1, 31} <= rem    # a full last step, a single valid key, a single masked key
    assert {101, 145, 170} <= set(C.COUNTS)  # the evaluator at 160^2, 192^2, 208^2
    # waves that project but hold no query exist below 193 tokens only; both kinds of count are present
    assert any(n <= 192 for n in C.COUNTS) and any(n > 192 for n in C.COUNTS)


def test_ordinary_inputs_are_computed_once_per_shape():
    a, b = C.ordinary(2, 33), C.ordinary(2, 33)
    assert all(x is y for x, y in zip(a, b))  # computed once, shared
    xn, w, bias = a
    assert xn.shape == (66, 384) and w.shape == (1152, 384) and bias.shape == (1152,)
    assert abs(xn.std().item() - 1) < 0.05 and abs(w.std().item() - 0.05) < 0.005 and abs(bias.std().item() - 0.1) < 0.02
    assert not torch.equal(C.ordinary(2, 33, seed=1)[0], xn)


@pytest.mark.parametrize("n", C.STRESS_COUNTS)
@pytest.mark.parametrize("recipe", C.RECIPES)
def test_stress_inputs_force_the_branch_they_claim(recipe, n):
    xn, w, b = C.stress(recipe, B, n)
    # Q and K select the head's input columns, no bias: the score of (i, j) is x_i . x_j over the head's 64 columns
    assert torch.equal(w[:384], torch.eye(384)) and torch.equal(w[384:768], torch.eye(384)) and not b[:768].any()
    s = C.raw_scores(xn, w, b, B)
    x5 = xn.double().reshape(B, n, C.HEADS, 64).permute(0, 2, 1, 3)
    assert torch.equal(s, x5 @ x5.transpose(-2, -1))
    # inside f16 range with room to spare: operands up to 10, raw scores up to 640 (80 after scaling by 1 / 8) - and large
    # enough that the maximum has to move: several times the lazy limit of 44.4
    assert xn.abs().max().item() <= 10.0
    assert 8 * C.lazy_limit(0.125) <= s.abs().max().item() <= 640.0
    nsteps = (n + 31) >> 5
    last_wave = (n - 1) >> 5
    for img in range(B):
        for head in range(C.HEADS):
            moves = C.replay_moves(s[img, head], 0.125)
            assert set(moves) == {(wv, t) for wv in range(last_wave + 1) for t in range(2) if t == 0 or wv * 32 + 16 < n}
            assert all(at[0] == 0 for at in moves.values())  # every query tile moves at step 0 (from -inf)
            later = {k: len(at) - 1 for k, at in moves.items()}
            if recipe == "rising":  # the maximum keeps moving after its first move
                assert all(v >= 1 for v in later.values())
                if n > 96:  # (65 tokens are three steps: one later move is all the limit leaves room for)
                    assert max(later.values()) >= 2, (img, head, moves)
            elif recipe == "one_tile":  # in one wave: a tile that stays where step 0 put it next to one that keeps moving
                for wv in range(last_wave + 1):
                    assert later[(wv, 0)] == 0, (img, head, wv, moves)
                assert later[(0, 1)] >= 1 and len(moves[(0, 1)]) >= 2, (img, head, moves)
                assert all(later[(wv, 1)] >= 1 for wv in range(last_wave + 1) if (wv, 1) in moves)
            else:  # "last": the maximum arrives in the final, masked step and nowhere between
                assert any(at[-1] == nsteps - 1 for at in moves.values()), (img, head, moves)
                assert all(set(at) <= {0, nsteps - 1} for at in moves.values())
    if recipe == "last":
        a, _ = C.amplitudes(recipe, n)
        assert a.argmax().item() == n - 1 and n - 32 * (nsteps - 1) == {197: 5, 193: 1, 65: 1}[n]  # valid keys of the last step
        assert n % 32 != 0  # so that step is a masked one


def test_one_tile_recipe_moves_tile_1_at_least_twice_somewhere():
    """at N = 197 the second tile of a wave moves at two later steps in some (image, head): the ballot of the still tile is
    taken more than once while its neighbour moves"""
    xn, w, b = C.stress("one_tile", B, 197)
    s = C.raw_scores(xn, w, b, B)
    best = max(len(at) for img in range(B) for head in range(C.HEADS)
               for (wv, t), at in C.replay_moves(s[img, head], 0.125).items() if t == 1)
    assert best >= 3


def test_replay_follows_the_laziness_constant():
    """the rule is `block maximum > running + LAZY_BITS / (scale log2 e)`: with a huge limit only step 0 moves, with none every
    rise does"""
    xn, w, b = C.stress("rising", B, 197)
    s = C.raw_scores(xn, w, b, B)[0, 0]
    assert abs(C.lazy_limit(0.125) - 44.3614) < 1e-3
    saved = C.LAZY_BITS
    try:
        C.LAZY_BITS = 1e9
        assert all(at == [0] for at in C.replay_moves(s, 0.125).values())
        C.LAZY_BITS = 0.0
        assert len(C.replay_moves(s, 0.125)[(0, 1)]) == 7
    finally:
        C.LAZY_BITS = saved


def test_references_agree_on_ordinary_inputs():
    xn, w, b = C.ordinary(2, 33)
    r64, r32 = C.ref(xn, w, b, 2, 0.125), C.ref_f32(xn, w, b, 2, 0.125)
    assert r64.dtype == torch.float64 and r32.dtype == torch.float32 and r64.shape == r32.shape == (66, 384)
    assert (r32.double() - r64).abs().max().item() <= 1e-5


def test_forward_rows_name_their_token_counts():
    assert [C.tokens_of(r) for r in C.FORWARD_ROWS] == C.FORWARD_TOKENS
    assert all(C.tokens_of(r) <= C.MAX_TOKENS for r in C.FORWARD_ROWS)  # or the "fused" pin falls back to the pair of launches
    assert all(r[1] * C.HEADS < 96 for r in C.FORWARD_ROWS)  # the automatic path would NOT take the fused kernel: the pin matters
    assert C.AUTO_ROW[1] * C.HEADS == 96 and C.tokens_of(C.AUTO_ROW) == 5
    assert {65, 101, 170} <= set(C.FORWARD_TOKENS)  # the evaluator's grids at 128^2, 160^2, 208^2


@pytest.mark.parametrize("row", C.FORWARD_ROWS, ids=[C.forward_id(r) for r in C.FORWARD_ROWS])
def test_forward_rows_meet_the_strict_gate_conditions(row):
    """the condition the edge rows of test_hip_forward.py state: |logit| <= 16 and the fp32 oracle within 5e-5 of its fp64 evaluation"""
    o32, o64 = C.oracle_row(row), C.oracle_row_f64(row)
    scale = o32["mask_logits"].abs().max().item()
    r64 = (o32["mask_logits"].double() - o64["mask_logits"]).abs().max().item()
    print(f"\n{C.forward_id(row)}: N={C.tokens_of(row)} |logit|max={scale:.2f} ref32-ref64={r64:.2e}")
    assert scale <= 16.0
    assert r64 <= 5e-5
