"""CPU tier: the rolling kernel's path table layout (c-ray_amd/csrc/cray_hip.hip: PathTab) changes addresses only.

The lean instantiations of k_pathtrace_roll (no node programs, no volumes) keep a path's words in three arrays — 64-B ray + shading parts,
16-B hit parts, 4-B instance words — instead of one 128-B record per path. The kernel emulation (tests/emu) is built a second time with
-DCRH_PATH_LEAN=0, which restores the 128-B record in every instantiation, and both libraries render the same fixtures: frames, the counters of
counter level 2 and the lanes the scheduler's steps served must be identical, and each frame must equal the reference's float buffer bit for bit.

Fixtures: the lean layout on scenes of many instances (spheres and meshes), with refraction and with emission; node programs and volumes (the
rare-features instantiations, which keep the 128-B record) must come out the same in both builds too. (The instance word has an array of its own
whatever the scene's instance and prim counts, so no scene takes another branch of the layout.)

The variant build and the child that renders the fixtures are tests/emu_variants.py's.
"""
import pytest

from emu_variants import build_variants, render_with_each


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    """(the emulation library as built, the same source with -DCRH_PATH_LEAN=0)"""
    return build_variants(tmp_path_factory.mktemp("lean0"), {"lean0": ["-DCRH_PATH_LEAN=0"]})


def test_lean_path_table_is_bit_identical_to_the_128_byte_record(libs):
    lean, wide = render_with_each(libs)
    for a, b in zip(lean, wide):
        assert a["kernel"].startswith("k_pathtrace_roll<2,4,"), a
        assert a == b, (a, b)
        assert a["ref_equal"] in (True, None), a
        assert a["counters"]["rays"] > 0
    # the lean layout was exercised (and the rare-features instantiations were reached too)
    assert any(",false," in r["kernel"] for r in lean) and any(",true," in r["kernel"] for r in lean), [r["kernel"] for r in lean]
