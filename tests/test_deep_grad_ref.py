"""The deep scenes of tests/deep_cases.py on the CPU: what every case must meet for tests/test_deep_grad_gpu.py to hold the
kernels' continuation rounds, group-list segments, own traversals and sample passes to float64, and that the comparison's
bound would catch the faults those paths can have.

Per case: at most a third of the pixels float32-sensitive (the upstream gradient is zero there), the candidate counts per
kernel tile and per group of 2x2 tiles that put the case on its path, stops, an alpha clamped at 0.99 behind other hits,
clamped and open colour channels. Counts: a Gaussian with a hit the blend may take on a ray of a tile is a candidate of
that tile under any cull, and no list is longer than the scene (deep_cases.hit_sets), so the bounds hold whatever the
renderer culls by. test_power plants six faults in copies of the reference's hit lists (deep_cases.planted) and reports by
what factor each misses the GPU tests' bound, 1e-3 M.
"""
import numpy as np
import pytest

import cor_f64 as F
import deep_cases as DC
import test_grad_f64 as S

TOL = S.TOL
CASES = pytest.mark.parametrize("case", DC.CASES, ids=DC.case_id)


@CASES
def test_scene_conditions(case):
    name, w, h, spp = case
    res = DC.sensitive(case)
    cn = res.counts
    has, per_ray = DC.hit_sets(case)
    n = has.shape[1]
    tw, th, lanes = DC.kernel_tile(spp)
    tiles, groups = DC.block_counts(case, tw, th), DC.block_counts(case, 2 * tw, 2 * th)
    layer = DC.scene(name)[5]
    print(f"{DC.case_id(case)}: {n} Gaussians, sensitive {res.near.mean():.2%} of the pixels; hits per ray "
          f"{per_ray.min()}..{per_ray.max()}; candidates per {tw}x{th} tile at least {tiles.min()}..{tiles.max()}, per group "
          f"at least {groups.min()}..{groups.max()}, at most {n}; {cn}")
    # the condition on the sensitive share, with and without SH rows (the same hits, no colour decisions)
    assert res.near.mean() <= 1.0 / 3.0
    bare = DC.sensitive(case, with_sh=False)
    assert bare.near.mean() <= res.near.mean() and bare.counts["clamped_behind"] == cn["clamped_behind"]
    # the path
    if name == "cut":  # every tile cut at 256, every group inside its first segment
        print(f"  margins: tiles {tiles.min() - DC.K_CAP} above 256, groups {DC.K_GCAP - n} below 896")
        assert tiles.min() > DC.K_CAP + 100 and n < DC.K_GCAP - 100
    elif name == "segment":  # every group in its second segment; 16 samples per pixel in the wave, so k_group_more runs
        print(f"  margins: groups {groups.min() - DC.K_GCAP} above 896, {DC.K_GLIST - n} below 1792")
        assert lanes >= 16 and groups.min() > DC.K_GCAP + 100 and n < DC.K_GLIST - 100 and tiles.min() > DC.K_GCAP
    elif name == "traverse":  # every tile past the group list's end
        print(f"  margins: tiles {tiles.min() - DC.K_GLIST} above 1792")
        assert lanes == 1 and tiles.min() > DC.K_GLIST + 100
    else:  # one pixel per lane, the samples in passes; more than one round per pass
        print(f"  margins: tiles {tiles.min() - DC.K_CAP} above 256")
        assert (tw, th, lanes) == (8, 8, 1) and spp > 64 and w <= 12 and h <= 10 and tiles.min() > DC.K_CAP + 40
    assert per_ray.min() > DC.K_CAP  # every ray's own list goes past the first round
    # the tiles' lists differ: the small Gaussians are candidates of some tiles and not of others
    small = has[:, slice(*layer["small"])].reshape(h, w, -1)
    first = small[:th, :tw].any((0, 1))
    assert first.any() and not first.all() and small.any((0, 1)).mean() > 0.8
    assert has[:, slice(*layer["faint"])].all()  # every faint Gaussian is a hit of every ray: alpha stays above 1/255
    # the events the comparison must reach
    assert cn["stopped_rays"] == w * h * spp  # every ray stops, in the opaque layer
    assert cn["clamped_behind"] >= 3
    assert 0.1 < cn["channels_clamped"] / cn["channels"] < 0.9
    assert cn["mean_alpha"] > 0.99


def _factors(case, fault):
    """the largest |faulty - true| / (TOL M) over the entries of the opacity and of the SH table, G as the GPU tests form it"""
    G, true, _ = DC.reference(case)
    with DC.planted(fault):
        wrong = F.gradients(DC.camera(case), *DC.model(case), G_rgba=G)
    out = []
    for field in ("opacity", "sh"):
        got, ref, M = getattr(wrong, field), getattr(true, field), getattr(true, "M_" + field)
        reached = M > 0
        out.append(float((np.abs(got - ref)[reached] / (TOL * M[reached])).max()))
    return out


FAULTS = [("drop256", ("cut", 24, 16, 1)), ("drop896", ("traverse", 24, 16, 1)), ("skip257", ("cut", 24, 16, 1)),
          ("twice", ("cut", 24, 16, 1)), ("pass_twice", ("passes", 12, 10, 80)), ("sweep_short", ("cut", 24, 16, 1)),
          ("sweep_short", ("traverse", 24, 16, 1))]


@pytest.mark.parametrize("fault,case", FAULTS, ids=lambda v: v if isinstance(v, str) else DC.case_id(v))
def test_power(fault, case):
    """Each planted fault misses the bound by the factors printed (measured: DESIGN.md section 5), ten at least on the
    opacity gradient, a resweep kind, and on the SH gradient. A pass counted twice adds one sample's terms to an entry that
    sums 80 samples' over every pixel the Gaussian meets: only an entry of few terms shows it. Those are the pins of the
    `passes` scene (deep_cases.scene), a few dozen hits each, the second sample's the largest; without them the opacity
    gradient missed the bound by 6.2 only."""
    assert case in DC.CASES
    f_o, f_sh = _factors(case, fault)
    if fault == "sweep_short":  # a fault of the resweep kinds: the SH gradient has one sweep
        f_sh = None
    print(f"{fault} on {DC.case_id(case)}: misses 1e-3 M by a factor of {f_o:.3g} (opacity)" +
          ("" if f_sh is None else f", {f_sh:.3g} (SH)"))
    assert f_o >= 10.0 and (f_sh is None or f_sh >= 10.0)


def test_planted_leaves_the_reference_as_it_was():
    case = DC.CASES[0]
    G, true, _ = DC.reference(case)
    with DC.planted("twice"):
        pass
    again = F.gradients(DC.camera(case), *DC.model(case), G_rgba=G)
    assert again.digest == true.digest and np.array_equal(again.opacity, true.opacity)
