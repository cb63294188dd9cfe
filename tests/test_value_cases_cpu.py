"""tests/value_cases.py on the CPU: the atlas and the poses cover every byte value at both frame sizes, the (scale,
bias) table reaches what each row is in it for and numpy agrees with torch on the CPU about all of it, and the JPEG frames
write the codes, and end on the bit counts, that tests/test_gpu_jpeg_codes.py and tests/test_jpeg_kernel_host.py need
them to -- so that those cannot pass on inputs that reach nothing."""
import numpy as np
import pytest
import torch

import jpeg_model as J
import value_cases as V
from gridworld_amd import render as R

# ---- observation side ----------------------------------------------------------------------------------------------


def test_the_atlas_is_accepted_and_its_tiles_hold_the_ramp_the_corners_and_noise():
    a = R.check_atlas(V.atlas())
    assert a.shape == (128, 128, 4) and (a[..., 3] == 255).all()
    for tid in (-1, 0, 1, 3, 4, 6):                                     # the two ground tiles and the scene's blocks
        tx, ty = R.TILES[tid]
        tile = a[128 - 32 * (ty + 1):128 - 32 * ty, 32 * tx:32 * tx + 32, :3].reshape(-1, 3).astype(int)
        ramp = tile[(tile[:, 0] == tile[:, 1]) & (tile[:, 1] == tile[:, 2])]
        assert set(ramp[:, 0].tolist()) == set(range(256))
        assert (V.luminance(ramp) == ramp[:, 0]).all()                  # the luminance of (v, v, v) is v
        assert set(map(tuple, V.CORNERS)) <= set(map(tuple, tile.tolist()))
        assert len(np.unique(tile, axis=0)) >= 1000                     # 256 + 8 + seeded noise


@pytest.mark.parametrize('size', V.SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_the_predicted_frames_cover_every_value(size):
    grid, poses = V.scene()
    assert 8 <= len(poses) <= 16 and (np.abs(poses[:, [0, 2]]) <= 10).all()
    assert (np.abs(poses[:, :3] - np.round(poses[:, :3])) > 5e-3).all()   # eyes off the integer lattice
    frames, clean = V.predicted(size)
    c = V.coverage(frames)
    print(f'{size}: {c["triples"]} distinct triples, {100 * clean:.2f} % of the pixels outside the boundary band')
    assert c['missing'] == [[], [], []] and c['missing_luminance'] == [] and c['triples'] >= V.MIN_TRIPLES
    assert V.covered(frames) and clean >= 0.98
    assert (size[0] * size[1] % 4 == 0) == (size == (64, 64))            # lanes of four at one size only


# what each row of V.ROWS must reach, counted by V.reaches() from the reference (exact counts)
REACH = (
    dict(inexact_products=247, negative=0), dict(negative=128), dict(negative=128),
    dict(inexact_products=247), dict(inexact_products=247),
    dict(negative=255, f32_neg_zero=0), dict(negative=255),
    dict(f16_ties=128), dict(bf16_ties=128),
    dict(f16_ties=20, f16_inf=1), dict(f16_max=1, f16_inf=0),
    dict(f16_subnormals=255), dict(f16_ties=128, f16_subnormals=254),
    dict(f32_subnormals=255), dict(f32_subnormals=255, negative=128),
    dict(f32_inf=254, f16_inf=255), dict(f32_neg_inf=254, f16_inf=256),
    dict(f32_neg_zero=1, negative=255),
)


@pytest.mark.parametrize('row', range(len(V.ROWS)), ids=[f'{s:g}*v{b:+g}' for s, b, _ in V.ROWS])
def test_every_row_reaches_what_it_is_for_and_numpy_agrees_with_torch_on_the_cpu(row):
    scale, bias, what = V.ROWS[row]
    got = V.reaches(scale, bias)
    for key, n in REACH[row].items():
        assert got[key] == n, (what, key, got)
    # torch on the CPU, as tests/obs_model.py computes it: mul, add, .to(dtype), each rounding once
    f = torch.arange(256, dtype=torch.uint8).to(torch.float32)
    f = torch.add(torch.mul(f, torch.tensor(scale, dtype=torch.float32)), torch.tensor(bias, dtype=torch.float32))
    for name in V.DTYPES:
        t = f.to(getattr(torch, name))
        bits = t.view({2: torch.int16, 4: torch.int32}[t.element_size()]).numpy().view(V.BITS[name])
        assert np.array_equal(bits, V.table(name, scale, bias)), (what, name)
    # the spec takes the row as it is (signed zero included) and rounds it to float32 like numpy
    spec = R.ObsSpec(torch.float32, scale=scale, bias=bias)
    obs = R.Obs(scale=spec.scale, bias=spec.bias)
    assert np.float32(obs.scale).tobytes() == np.float32(scale).tobytes()
    assert np.float32(obs.bias).tobytes() == np.float32(bias).tobytes()


def test_the_table_has_the_rows_of_the_three_usual_normalisations_first_and_bf16_never_wraps():
    assert [r[:2] for r in V.ROWS[:3]] == [(1 / 255, 0.0), (2 / 255, -1.0), (1.0, -128.0)] and len(V.ROWS) == 18
    # the carry of the bf16 rounding at the top of the f32 range: the largest finite f32 rounds to +-inf, not to 0
    top = np.array([np.finfo(np.float32).max, -np.finfo(np.float32).max, np.inf, -np.inf, np.nan], np.float32)
    assert V.bf16_bits(top).tolist() == [0x7f80, 0xff80, 0x7f80, 0xff80, 0x7fc0]


def test_expected_is_planes_through_the_table_tiled_over_the_stack():
    frames = V.predicted((64, 64))[0][:2]
    spec = R.ObsSpec(torch.float16, gray=True, stack=3, scale=257.0)
    e = V.expected(frames, spec)
    assert e.shape == (2, 3, 64, 64) and e.dtype == np.uint16
    lum = V.luminance(frames)
    assert np.array_equal(e[:, 0], V.table('float16', 257.0, 0.0)[lum]) and np.array_equal(e[:, 0], e[:, 2])
    rgb = V.expected(frames, R.ObsSpec(torch.uint8, stack=2))
    assert rgb.shape == (2, 6, 64, 64) and np.array_equal(rgb[:, 3:].transpose(0, 2, 3, 1), frames)
    # the model the other observation tests use, on the CPU, says the same
    import obs_model as OM
    for kw in (dict(dtype=torch.bfloat16, scale=1.0, bias=256.0),
               dict(dtype=torch.float32, gray=True, scale=2.0 ** -149)):
        s = R.ObsSpec(stack=2, **kw)
        want = OM.bits(OM.observe(torch.from_numpy(frames), None, None, s)).numpy()
        assert np.array_equal(V.expected(frames, s), want.view(V.expected(frames, s).dtype))


# ---- JPEG side -----------------------------------------------------------------------------------------------------
# The AC symbols (run << 4 | size) that no frame of value_cases writes, and why.  All have size 10: a coefficient of at
# least 512 quantisation steps.  An 8 x 8 block of 8-bit pixels holds one only where the divisor is 1 to 3 (qualities
# 100 to 95) and the basis function's peak, amplitude / 8 in the first row or column and amplitude / 4 elsewhere (a
# little less where no sample falls on the peak), stays within 127 of the block's mean.
UNREACHED = {
    # luma: 27 positions hold a size-10 coefficient at quality 100, but no k with k - 1 = 7 (mod 16) is among them
    # (8, 24, 40, 56), and at k = 20, 52 (run 3) and k = 28 (run 11) the rounding of the pixels leaves a second, small
    # coefficient in the block, and the run comes out shorter
    0: {0x3a, 0x7a, 0xba},
    # chroma: the amplitude also passes the inverse colour transform (R = Y + 1.402 Cr, B = Y + 1.772 Cb), which only
    # Cr survives, and only with the three basis functions whose 64 samples all have one magnitude (u, v in {0, 4}):
    # k = 10, 14, 39, the runs 9, 13 and 6.  Every other run with size 10 is out of reach
    1: {r << 4 | 10 for r in range(16)} - {0x6a, 0x9a, 0xda},
}


@pytest.fixture(scope='module')
def counts():
    return {name: V.merge([V.count(J.coefficients(f, q)) for f in frames]) for name, frames, q in V.jpeg_batches()}


def test_the_synthesised_frames_reach_the_ac_symbols_the_long_codes_and_the_zrl_chains(counts):
    for q in V.QUALITIES:
        f = V.synthesised(q)
        assert f.shape[1:] == (8 * V.FRAME_BLOCKS // 8, 64, 3) and f.dtype == np.uint8 and 3 <= len(f) <= 8
    total = V.merge(counts.values())
    for tab, floor in ((0, 150), (1, 138)):
        reached = {s for t, kind, s in total['symbols'] if t == tab and kind == 'ac'}
        print(f'table {tab}: {len(reached)} of 162 AC symbols, longest code {total["longest"][tab]} bits')
        assert len(reached) >= floor
        assert set(J.AC_CODES[tab]) - reached == UNREACHED[tab]
        assert total['longest'][tab] == 26                                # put() is documented for 26 bits
    assert total['zrl'] == {1, 2, 3}
    assert counts['synthesised q100']['no_eob'] >= 100                    # last non-zero coefficient at k = 63
    blocks = sum(len(V.synthesised(q)) for q in V.QUALITIES) * V.FRAME_BLOCKS
    print(f'{blocks} blocks in {blocks // V.FRAME_BLOCKS} frames; {total["no_eob"]} blocks without an EOB')


def test_the_dc_frames_reach_every_category_in_both_signs(counts):
    f = V.dc_frames()
    assert f.shape == (4, 64, 64, 3)
    for a, b in V.CHECKER_PAIRS:
        assert any((fr[0, 0] == a).all() and (fr[0, 8] == b).all() and (fr[8, 0] == b).all() for fr in f[:3])
    want = {(0, 0)} | {(c, s) for c in range(1, 12) for s in (-1, 1)}
    for tab in (0, 1):
        got = {(c, s) for t, c, s in counts['dc frames']['dc_signed'] if t == tab}
        assert got == want and len(got) == 23, (tab, sorted(want - got))
    # the checkerboards alone hold the largest category of both tables
    three = V.merge([V.count(J.coefficients(fr, 100)) for fr in f[:3]])
    assert {(0, 11, 1), (0, 11, -1), (1, 11, 1), (1, 11, -1)} <= three['dc_signed']


def test_the_three_bit_counts_at_the_window_boundary():
    al = V.aligned()
    # the whole scan is one window: the last chunk ends on the boundary with no padding
    f, q = al['scan-ends-on-window']
    assert f.shape == (360, 416, 3) and (f == 200).all() and q == 50
    ends = V.chunk_end_bits(f, q)
    assert len(ends) == 37 and 52 * 45 == 2340 and ends[-1] == V.WINDOW_BITS == 32768 and ends[-1] % 8 == 0
    # a chunk that is not the last ends on the boundary: the next one starts an empty window
    f, q = al['chunk-ends-on-window']
    assert f.shape == (304, 512, 3) and q == 60 and (f[8:] == 128).all() and (f[:, 8:] == 128).all()
    ends = V.chunk_end_bits(f, q)
    assert len(ends) == 38 and ends[35] == V.WINDOW_BITS and ends[-1] == 34560
    # the same kind of frame, but a code begins in front of the boundary and ends behind it, in the slack words
    f, q = al['code-straddles-window']
    assert f.shape == (304, 512, 3) and q == 60 and not np.array_equal(f, al['chunk-ends-on-window'][0])
    cum = V.cumulative_bits(f, q)
    i = int(np.searchsorted(cum, V.WINDOW_BITS))
    print(f'the straddling code: bits {cum[i - 1]}..{cum[i]} of {cum[-1]}')
    assert cum[i - 1] < V.WINDOW_BITS < cum[i] < cum[-1] and V.WINDOW_BITS not in cum
    assert V.WINDOW_BITS not in V.chunk_end_bits(f, q)
