"""Edge configs of the HiFi-GAN generator, their cases and a restatement of the plan's shape rules (helper of
test_hifigan_edge.py and tests/golden/make_golden_hifigan_edge.py; TEST INFRASTRUCTURE ONLY).

The seven ``hifigan_*.npz`` goldens share num_mels 80, channel counts that are multiples of 32, ``kernel = 2 x rate`` upsampling,
resblock kernels 3 .. 11 with halos <= 72 and 2 or 3 resblocks per stage.  The four configs here are what csrc/hifigan_plan.h
accepts beyond that; they are kept OUT of ``synthetic.HIFIGAN_CONFIGS`` (tests iterate that dict) and their fixtures are
``hgedge_<config>.npz`` (``hifigan_restatement.golden_cases()`` takes every ``hifigan_*.npz``).

``plan(cfg, esz)`` restates ``make_hg_plan`` / ``hg_add_layer`` and ``launch_shape`` the narrow rule of ``hg_launch``: block
heights, the K chunk with the rule that chose it, the column tile of a launch.  From them ``edges_reached`` tells which
column-tile edges a frame count reaches, and test_hifigan_edge.py asserts that CASES reaches every edge a frame count up to
MAX_FRAMES can reach - a later edit of the plan that moves an edge away from the cases fails there.
"""
import collections
import os

import numpy as np

from cookietts_amd import synthetic

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAX_FRAMES = 130

CONFIGS = {
    # 24 -> 12 -> 6 channels: every Cin ragged against the K chunk, cout = 6 (cout % 4 != 0, M = 6 ragged against rows of 4),
    # odd rate 3 with a 5-tap kernel, then kernel == rate
    "r24": synthetic.hifigan_config(num_mels=13, upsample_initial_channel=24, upsample_rates=(3, 2), upsample_kernel_sizes=(5, 2),
                                    resblock="1", resblock_kernel_sizes=(3, 5), resblock_dilation_sizes=((1, 2, 4), (1, 3, 5)),
                                    hop_size=6),
    # 80 -> 40 -> 20 channels: halos 128, 120, 126; M = 200 (two 128-row blocks, the second partly empty), 80, 40, 20
    "r80": synthetic.hifigan_config(num_mels=20, upsample_initial_channel=80, upsample_rates=(5, 4), upsample_kernel_sizes=(11, 6),
                                    resblock="2", resblock_kernel_sizes=(3, 11, 7), resblock_dilation_sizes=((1, 64), (1, 12), (2, 21)),
                                    hop_size=20),
    # rate 1, kernel 1, one resblock per stage
    "k1": synthetic.hifigan_config(num_mels=80, upsample_initial_channel=40, upsample_rates=(1,), upsample_kernel_sizes=(3,),
                                   resblock="1", resblock_kernel_sizes=(1,), resblock_dilation_sizes=((1, 3, 5),), hop_size=1),
    # four resblocks per stage, 16 -> 8 -> 4 -> 2 channels (Cin <= the low K chunk after conv_pre, cout = 2), halo 128 with k = 9
    "k4": synthetic.hifigan_config(num_mels=7, upsample_initial_channel=16, upsample_rates=(2, 2, 2), upsample_kernel_sizes=(2, 4, 6),
                                   resblock="2", resblock_kernel_sizes=(1, 3, 5, 9),
                                   resblock_dilation_sizes=((1, 2), (2, 6), (3, 12), (1, 16)), hop_size=8),
}

# (batch, frames, seed) per config.  Every case has two or three different items; one B = 3 case per config.  Frames: 1 and 2
# (shorter than conv_pre's left halo, shorter than one float4), all four residues of frames % 4, and for every layer a length
# just past a column-tile edge (L > BN, 1 <= L % BN <= 4) and one on or just below it (L % BN == 0 or >= BN - 4) wherever a
# frame count <= MAX_FRAMES reaches one - test_edge_cases_meet_the_conditions derives that set from the plan.
CASES = {
    # stage lengths 3 f and 6 f on 256-column tiles (M <= 32), ups.0 (M = 36) on 128: 43 -> 258 = 256 + 2; 85 -> 255, 510;
    # 86 -> 258, 516 = 2 x 256 + 4; 128 -> ups.0 on its tile, 768 = 3 x 256; 129 -> ups.0 one past
    "r24": [(2, 1, 201), (2, 2, 201), (3, 7, 201), (2, 43, 201), (2, 85, 201), (2, 86, 201), (2, 128, 201), (2, 129, 201)],
    # conv_pre / ups.0 (columns f) and ups.1 (5 f) on 64-column tiles, the 40-channel convs (5 f) on 128, the 20-channel ones
    # (20 f) on 256: 13 -> 65, 260; 26 -> 130; 51 -> 255, 1020; 64 / 128 -> every layer on its tile; 65 -> conv_pre one past
    "r80": [(2, 1, 202), (2, 2, 202), (3, 7, 202), (2, 13, 202), (2, 26, 202), (2, 51, 202), (2, 64, 202), (2, 65, 202),
            (2, 128, 202)],
    # rate 1: every length is f; only conv_pre (M = 40, 128-column tiles) reaches an edge by 130 frames
    "k1": [(2, 1, 205), (2, 2, 205), (3, 7, 205), (2, 128, 205), (2, 129, 205)],
    # stage lengths 2 f, 4 f, 8 f on 256-column tiles: 32 -> 256; 65 -> 260; 127 -> 254, 508; 128 -> 256, 512, 1024; 129 -> 258, 516
    "k4": [(2, 1, 205), (2, 2, 205), (3, 7, 205), (2, 32, 205), (2, 65, 205), (2, 127, 205), (2, 128, 205), (2, 129, 205)],
}

HG_MAX_HALO = 128
HG_LDS_MAX = 64 * 1024
HG_LDS_KC16 = 40 * 1024
HG_NARROW_BELOW = 1024

Layer = collections.namedtuple("Layer", "name kind stage Cin M cout up ku ntap dil left MT WM BM BN MB KC kc_rule nch esz")


def case_name(batch, frames):
    return f"b{batch}_f{frames}"


def _lds_bytes(esz, ntap, KC, BM, bn, dil, left):
    if esz == 2:
        return (ntap * KC * BM + KC * (bn + (ntap - 1) * dil)) * 2
    aleft = (left + 3) & ~3
    xw = (bn + (ntap - 1) * dil - left + aleft + 3) & ~3
    return (ntap * KC * BM + KC * xw) * 4


def plan(cfg, esz=4):
    """The layer list of ``make_hg_plan`` (esz 4: fp32 and split bf16, esz 2: IEEE half) in launch-table order: conv_pre, per
    stage ups.i and its resblocks' convs in module order, conv_post.  ``stage`` counts the upsamplings in front of the layer's
    column domain (a transposed conv's columns are its INPUT's).  ``kc_rule``: "hi", or why the low chunk was taken - "cin"
    (Cin <= kc_lo) or "lds" (the two LDS images at the high chunk exceed HG_LDS_KC16)."""
    layers = []
    kc_hi = 32 if esz == 2 else 16
    kc_lo = kc_hi // 2

    def add(name, kind, stage, Cin, M, cout, up, ku, ntap, dil, left):
        MT, WM = (1, 1) if M <= 32 else (2, 1) if M <= 64 else (2, 2)
        BM, BN = 32 * MT * WM, 64 * (4 // WM)
        KC, rule = kc_hi, "hi"
        if Cin <= kc_lo:
            KC, rule = kc_lo, "cin"
        elif _lds_bytes(esz, ntap, kc_hi, BM, BN, dil, left) > HG_LDS_KC16:
            KC, rule = kc_lo, "lds"
        assert _lds_bytes(esz, ntap, KC, BM, BN, dil, left) <= HG_LDS_MAX, name
        layers.append(Layer(name, kind, stage, Cin, M, cout, up, ku, ntap, dil, left, MT, WM, BM, BN, -(-M // BM), KC, rule,
                            -(-Cin // KC), esz))

    n_k = len(cfg["resblock_kernel_sizes"])
    steps = 3 if cfg["resblock"] == "1" else 2
    C = cfg["upsample_initial_channel"]
    add("conv_pre", "conv", 0, cfg["num_mels"], C, 0, 1, 0, 7, 1, 3)
    for i, (u, ku) in enumerate(zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"])):
        pad = (ku - u) // 2
        left, jhi = (ku - 1 - pad) // u, (u - 1 + pad) // u
        add(f"ups.{i}", "convt", i, C, u * (C // 2), C // 2, u, ku, left + jhi + 1, 1, left)
        C //= 2
        for j, (k, dil) in enumerate(zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"])):
            p = f"resblocks.{i * n_k + j}"
            for m in range(steps):
                assert (k - 1) * dil[m] <= HG_MAX_HALO
                add(f"{p}.convs1.{m}" if cfg["resblock"] == "1" else f"{p}.convs.{m}", "conv", i + 1, C, C, 0, 1, 0, k, dil[m],
                    (k - 1) // 2 * dil[m])
            if cfg["resblock"] == "1":
                for m in range(3):
                    add(f"{p}.convs2.{m}", "conv", i + 1, C, C, 0, 1, 0, k, 1, (k - 1) // 2)
    add("conv_post", "conv", len(cfg["upsample_rates"]), C, 1, 0, 1, 0, 7, 1, 3)
    return layers


def packed_bytes(cfg, esz=4):
    """``p.packed_bytes`` of the library's plan from this one: per layer the weight block [MB][nch][ntap][KC][BM] of ``esz``-byte
    elements and the fp32 bias block [MB * BM], each rounded up to 256 bytes.  Equal to the library's size query only if the
    block heights, tap counts and K chunks of the two plans agree."""
    def align(v):
        return (v + 255) // 256 * 256
    return sum(align(l.MB * l.nch * l.ntap * l.KC * l.BM * esz) + align(l.MB * l.BM * 4) for l in plan(cfg, esz))


def columns(cfg, layer, frames):
    """Column count of a layer's launch."""
    return frames * int(np.prod(cfg["upsample_rates"][:layer.stage], dtype=np.int64))


def launch_shape(layer, L, batch):
    """(MT, WM, BN, workgroups of the plan's shape) of ``hg_launch``: a launch that would start fewer than HG_NARROW_BELOW
    workgroups of the plan's shape takes the half-width block of the same height (and starts twice as many, or one fewer)."""
    MT, WM, BN = layer.MT, layer.WM, layer.BN
    wide = layer.MB * (-(-L // BN)) * batch
    if layer.BM >= 64 and wide < HG_NARROW_BELOW:
        MT, WM, BN = 1, WM * 2, BN // 2
    return MT, WM, BN, wide


def edges_reached(cfg, batch, frames, esz=4):
    """{(layer name, "past" | "at")}: the layer's column count is just past a tile edge (L > BN, 1 <= L % BN <= 4) / on or just
    below one (L % BN == 0 or L % BN >= BN - 4)."""
    out = set()
    for l in plan(cfg, esz):
        L = columns(cfg, l, frames)
        BN = launch_shape(l, L, batch)[2]
        if L > BN and 1 <= L % BN <= 4:
            out.add((l.name, "past"))
        if L % BN == 0 or L % BN >= BN - 4:
            out.add((l.name, "at"))
    return out


def state_dict(key, seed):
    return synthetic.hifigan_state_dict(CONFIGS[key], seed=seed)


def mel(key, batch, frames, seed):
    """Items differ (one draw of [batch, num_mels, frames])."""
    return synthetic.synthetic_mel(batch, frames, CONFIGS[key]["num_mels"], seed=seed + 1000 * frames + batch)


def fixture_path(key):
    return os.path.join(GOLDEN, f"hgedge_{key}.npz")


def load_cases(key):
    """[(case name, dict(seed, mel, audio, ref_fp32_vs_fp64, audio_half, ref_half_vs_fp32))] in CASES order."""
    z = np.load(fixture_path(key))
    out = []
    for batch, frames, _ in CASES[key]:
        name = case_name(batch, frames)
        out.append((name, {f: z[f"{name}.{f}"] for f in ("seed", "mel", "audio", "ref_fp32_vs_fp64", "audio_half", "ref_half_vs_fp32")}))
    return out
