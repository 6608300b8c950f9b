"""Inputs of the fused QKV + attention tests, shared by test_qkv_attention_cases_cpu.py (checks the inputs) and
test_hip_qkv_attention.py / test_hip_forward.py (check the kernel): the token counts at which qkv_attention.hip changes what
a wave does, three inputs that force its lazy running-maximum rescale, the fp64 reference of the operation, a replay of the
kernel's rescale rule on fp64 scores, and the forward rows that reach the kernel at small token grids.

What the kernel does with a token count N (qkv_attention.hip): wave w owns tokens 32w .. 32w + 31 as two 16-token tiles and
takes the second only if 32w + 16 < N; a wave with 32w >= N projects (its K / V rows repeat the last token) and holds no
query; keys come in (N + 31) >> 5 steps of 32, and only the last step masks keys >= N.  Per step a query tile moves its running
maximum only when one of its queries' block maximum exceeds the running one by more than 8 / (scale log2 e)."""
import functools
import math

import torch

HEADS, HEAD_DIM, EMBED = 6, 64, 384
MAX_TOKENS = 208
LAZY_BITS = 8.0  # qkv_attention.hip: `lim = 8.0f / cs`, cs = scale * log2(e) - p <= 2^8 between two moves of the maximum

# 32w + 16 / + 17: the wave's second tile appears;  32w / 32w + 1: a wave without a query, and a new key step;
# 32s + 15 / + 16 / + 17: the last 16-key tile of the last step partly / wholly masked / the next one started;
# 101, 145, 170: the evaluator's grids at 160^2, 192^2, 208^2 (65 = 128^2 has a case of its own in the parity test)
COUNTS = [2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 95, 96, 97, 99, 101, 128, 129, 145, 160, 161, 170, 176, 177, 191, 192,
          196, 207]


def ref(xn, w, b, B, scale):
    M = xn.shape[0]
    n = M // B
    qkv = (xn.double() @ w.double().T + b.double()).reshape(B, n, 3, 6, 64).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    attn = torch.softmax((q @ k.transpose(-2, -1)) * scale, dim=-1)
    return (attn @ v).transpose(1, 2).reshape(M, 384)


def ref_f32(xn, w, b, B, scale):
    """the same operation in torch fp32 on the CPU: the witness of what fp32 arithmetic loses on these inputs"""
    M = xn.shape[0]
    n = M // B
    qkv = (xn @ w.T + b).reshape(B, n, 3, 6, 64).permute(2, 0, 3, 1, 4)
    attn = torch.softmax((qkv[0] @ qkv[1].transpose(-2, -1)) * scale, dim=-1)
    return (attn @ qkv[2]).transpose(1, 2).reshape(M, 384)


@functools.lru_cache(maxsize=None)
def ordinary(B, n, seed=0, wstd=0.05):
    """unit-variance xn, weight std wstd, bias std 0.1 -> (xn (B n, 384), w (1152, 384), b (1152)) float32"""
    g = torch.Generator().manual_seed(5000 + 1000 * seed + n)
    xn = torch.randn(B * n, EMBED, generator=g)
    w = torch.randn(3 * EMBED, EMBED, generator=g) * wstd
    b = torch.randn(3 * EMBED, generator=g) * 0.1
    return xn, w, b


# ---- inputs that force the rescale branch ------------------------------------------------------------------------------------
RECIPES = ("rising", "one_tile", "last")
STRESS_COUNTS = (197, 193, 65)


def amplitudes(recipe, n):
    """a_j of the recipe, and which tokens are the weak ones of `one_tile`"""
    weak = torch.zeros(n, dtype=torch.bool)
    if recipe == "last":
        a = torch.full((n,), 0.7)
        a[n - 1] = 2.5
    else:
        a = torch.linspace(0.5, 2.5, n)
        if recipe == "one_tile":
            weak = (torch.arange(n) % 32) < 16
            a = torch.where(weak, torch.tensor(0.3), a)
    return a, weak


@functools.lru_cache(maxsize=None)
def stress(recipe, B, n):
    """Q and K of every head select that head's 64 input columns (identity rows, zero bias), so the raw score of query i and
    key j is x_i . x_j over those columns; tokens are a_j u + 0.05 noise with one u ~ N(0, I) per image, so the score is about
    64 a_i a_j: it follows the amplitudes.  V: random weights of std 0.05, bias std 0.1."""
    assert recipe in RECIPES
    g = torch.Generator().manual_seed(7000 + 10 * n + RECIPES.index(recipe))
    a, _ = amplitudes(recipe, n)
    u = torch.randn(B, 1, EMBED, generator=g)
    xn = (a[None, :, None] * u + 0.05 * torch.randn(B, n, EMBED, generator=g)).reshape(B * n, EMBED).contiguous()
    w = torch.zeros(3 * EMBED, EMBED)
    w[:EMBED] = torch.eye(EMBED)
    w[EMBED:2 * EMBED] = torch.eye(EMBED)
    w[2 * EMBED:] = torch.randn(EMBED, EMBED, generator=g) * 0.05
    b = torch.zeros(3 * EMBED)
    b[2 * EMBED:] = torch.randn(EMBED, generator=g) * 0.1
    return xn, w, b


def raw_scores(xn, w, b, B):
    """q k^T before scaling, fp64, (B, heads, n, n)"""
    n = xn.shape[0] // B
    qk = (xn.double() @ w[:2 * EMBED].double().T + b[:2 * EMBED].double()).reshape(B, n, 2, HEADS, HEAD_DIM).permute(2, 0, 3, 1, 4)
    return qk[0] @ qk[1].transpose(-2, -1)


def lazy_limit(scale):
    return LAZY_BITS / (scale * math.log2(math.e))


def replay_moves(s, scale):
    """The kernel's running-maximum rule replayed on raw scores s (n, n) of one (image, head):  -> {(wave, tile): [steps at
    which the tile moved]}.  Per query a running maximum (-inf at the start); at every 32-key step the tile moves - every query
    of it takes max(running, block maximum) - when ANY of its queries' block maximum exceeds running + limit.  Keys >= n do
    not exist here (the kernel masks them); query rows >= n repeat the last token, which sits in the same tile."""
    n = s.shape[0]
    lim = lazy_limit(scale)
    nsteps = (n + 31) >> 5
    moves = {}
    for wave in range((n + 31) >> 5):
        for tile in range(2 if wave * 32 + 16 < n else 1):
            q0 = wave * 32 + tile * 16
            rows = s[q0:min(q0 + 16, n)]
            m = torch.full((rows.shape[0],), -math.inf, dtype=s.dtype)
            at = []
            for stp in range(nsteps):
                c = rows[:, stp * 32:min(stp * 32 + 32, n)].max(dim=1).values
                if bool((c > m + lim).any()):
                    m = torch.maximum(m, c)
                    at.append(stp)
            moves[(wave, tile)] = at
    return moves


# ---- forward rows: (patch, B, H, W, n_queries, decoder layers, seed), "calib" weights, synthetic_images(900 + seed) ------------
# token counts 99, 101, 208, 5, 170, 100, 2, 65, 157.  Seed 10 at 128^2 gives |logit| 16.5: not usable under the |logit| <= 16 rule.
FORWARD_ROWS = [
    (16, 3, 97, 211, 20, 2, 2),
    (16, 2, 160, 160, 20, 2, 6),
    (16, 2, 144, 368, 20, 2, 7),
    (16, 2, 32, 32, 20, 2, 4),
    (16, 2, 208, 208, 20, 2, 8),
    (8, 2, 72, 88, 20, 2, 3),
    (16, 2, 16, 16, 20, 2, 9),
    (16, 2, 128, 128, 20, 2, 13),
    (16, 2, 192, 208, 20, 2, 14),
]
FORWARD_TOKENS = [99, 101, 208, 5, 170, 100, 2, 65, 157]
AUTO_ROW = (16, 16, 32, 32, 20, 2, 4)  # B * 6 = 96 workgroups: the first batch the automatic path gives to the fused kernel


def forward_id(row):
    return "-".join(str(v) for v in row)


def tokens_of(row):
    """tokens per image as the encoder sees them: the patches of the image padded up to the patch size, and the cls token"""
    patch, _, H, W = row[:4]
    return -(-H // patch) * -(-W // patch) + 1


def forward_inputs(row):
    """(state_dict, images (B, 3, H, W) float32 tensor) of a row"""
    from selfmask_amd import synthetic_images, synthetic_state_dict
    patch, B, H, W, nq, L, seed = row
    sd = synthetic_state_dict(seed, "calib", n_queries=nq, patch_size=patch, n_decoder_layers=L, use_binary_classifier=True)
    return sd, torch.from_numpy(synthetic_images(900 + seed, (B, 3, H, W)))


@functools.lru_cache(maxsize=None)
def oracle_row(row, images=None):
    """the CPU oracle's fp32 forward of a row (of the listed images only, if given); computed once per process"""
    from oracle import selfmask_oracle as O
    sd, x = forward_inputs(row)
    if images is not None:
        x = x[list(images)]
    return O.forward(x, sd, row[0], n_layers=row[5])


def oracle_row_f64(row):
    from oracle import selfmask_oracle as O
    sd, x = forward_inputs(row)
    return O.forward(x.double(), O.cast_state(sd, torch.float64), row[0], n_layers=row[5])
