"""CPU: registers, scratch and LDS of the NORM_HAMMING2 kernels (csrc/hamming2.hip: ham2_prep_kernel, ham2_sweep_kernel<KTOP, KS>,
ham2_knnk_kernel<K, PK>, radius_ham2_kernel<FILL, KS>, ham2_radius_limits_kernel), read from the code object's metadata of the
unit cross-compiled with the product's flags: no spilled VGPRs, no scratch, LDS within the CU's 160 KiB; the instantiation
counts DESIGN.md states; and the `hamming` and `radius` units keep their kernels under their names and counts."""
import os
import re

import pytest

import isa_read as R

pytestmark = pytest.mark.skipif(not R.have_hipcc(), reason="needs hipcc to cross-compile csrc/hamming2.hip")

LDS_MAX = 163840
COUNTS = {"ham2_prep_kernel": 1, "ham2_sweep_kernel": 12, "ham2_knnk_kernel": 24, "radius_ham2_kernel": 12, "ham2_radius_limits_kernel": 1}


def _named(md, base):
    return {n: m for n, m in md.items() if re.match(r"_ZN2fm\d+%s(I|E)" % base, n)}


@pytest.fixture(scope="module")
def md(tmp_path_factory):
    return R.metadata(R.isa("hamming2", tmp_path_factory))


def test_no_spills_no_scratch_and_lds_fits(md):
    assert len(md) == sum(COUNTS.values()), sorted(md)
    for name, m in md.items():
        print(name, m["vgpr_count"], m["group_segment_fixed_size"])
        assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
        assert m["group_segment_fixed_size"] <= LDS_MAX, (name, m)
        assert m["vgpr_count"] <= 512 and m["max_flat_workgroup_size"] in (256, 1024), (name, m)


def test_instantiations_are_what_design_md_states(md):
    for base, count in COUNTS.items():
        assert len(_named(md, base)) == count, (base, sorted(_named(md, base)))
    sweep = sorted(re.search(r"ILi(\d)ELi(\d)E", n).groups() for n in _named(md, "ham2_sweep_kernel"))
    assert sweep == sorted((str(kt), str(ks)) for kt in (1, 2) for ks in range(1, 7))
    knnk = sorted(re.search(r"ILi(\d)ELi(\d)E", n).groups() for n in _named(md, "ham2_knnk_kernel"))
    assert knnk == sorted((str(k), str(pk)) for k in range(3, 9) for pk in range(1, 5))
    rad = sorted(re.search(r"ILb([01])ELi(\d)E", n).groups() for n in _named(md, "radius_ham2_kernel"))
    assert rad == sorted((f, str(ks)) for f in "01" for ks in range(1, 7))
    # two stages of 128 rows at a pitch of 64 KS + 16 bytes: the sweeps' LDS, by K steps
    for base in ("ham2_sweep_kernel", "radius_ham2_kernel"):
        for n, m in _named(md, base).items():
            ks = int(re.search(r"ELi(\d)E", n).group(1))
            assert m["group_segment_fixed_size"] == 2 * 128 * (64 * ks + 16), (n, m)
    design = open(os.path.join(R.ROOT, "DESIGN.md")).read()
    sect = design.split("**K11b")[1]
    for base, count in COUNTS.items():
        assert re.search(r"`%s[^`]*`[^|\n]*\|\s*%d\s*\|" % (base, count), sect), base
    assert "102,400" in sect or "102400" in sect


def test_hamming_and_radius_units_keep_their_pinned_counts(tmp_path_factory):
    ham = R.metadata(R.isa("hamming", tmp_path_factory))
    assert len(_named(ham, "ham_sweep_kernel")) == 8 and len(_named(ham, "ham_self_kernel")) == 4
    assert not any("ham2" in n for n in ham)
    rad = R.metadata(R.isa("radius", tmp_path_factory))
    assert len(_named(rad, "radius_ham_kernel")) == 8 and len(_named(rad, "rmask_ham_kernel")) == 8
    assert not any("ham2" in n for n in rad)
