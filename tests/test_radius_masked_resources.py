"""CPU: registers and scratch of the masked radius sweeps (csrc/radius.hip through radius_sweeps.inc: rmask_i8_kernel,
rmask_f16_kernel, rmask_ham_kernel<FILL, 1 .. 4>, rmask_wide_kernel<FILL, 5 .. 8>), read from the code object's metadata: no
scratch and no spills in any of the twenty, count and fill; and the unmasked sweeps are still there under their names."""
import re

import pytest

import isa_read as R

pytestmark = pytest.mark.skipif(not R.have_hipcc(), reason="needs hipcc to cross-compile csrc/radius.hip")


def _named(md, base):
    return {n: m for n, m in md.items() if re.match(r"_ZN2fm\d+%sI" % base, n)}


def _clean(name, m):
    print(name, m)
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, name
    assert m["vgpr_count"] <= 512 and m["max_flat_workgroup_size"] == 256, name


def test_masked_sweeps_have_no_scratch_and_no_spills(tmp_path_factory):
    md = R.metadata(R.isa("radius", tmp_path_factory))
    for base in ("rmask_i8_kernel", "rmask_f16_kernel"):
        ks = _named(md, base)
        assert sorted(re.search(r"ILb([01])E", n).group(1) for n in ks) == ["0", "1"], base
        for n, m in ks.items():
            _clean(n, m)
    for base, steps in (("rmask_ham_kernel", (1, 2, 3, 4)), ("rmask_wide_kernel", (5, 6, 7, 8))):
        ks = _named(md, base)
        assert sorted(re.search(r"ILb([01])ELi(\d)E", n).groups() for n in ks) == sorted((f, str(k)) for f in "01" for k in steps), base
        for n, m in ks.items():
            _clean(n, m)
            if base == "rmask_wide_kernel":
                assert m["group_segment_fixed_size"] == 0 and m["vgpr_count"] <= 256, n      # no LDS; two waves per SIMD
    # the masked integer and float32 sweeps keep the unmasked sweeps' LDS
    for a, b in (("rmask_i8_kernel", "radius_i8_kernel"), ("rmask_f16_kernel", "radius_f16_kernel"), ("rmask_ham_kernel", "radius_ham_kernel")):
        assert sorted(m["group_segment_fixed_size"] for m in _named(md, a).values()) == \
               sorted(m["group_segment_fixed_size"] for m in _named(md, b).values())


def test_unmasked_sweeps_keep_their_names_and_counts(tmp_path_factory):
    md = R.metadata(R.isa("radius", tmp_path_factory))
    assert len(_named(md, "radius_i8_kernel")) == 2 and len(_named(md, "radius_f16_kernel")) == 2
    assert len(_named(md, "radius_ham_kernel")) == 8 and len(_named(md, "radius_wide_kernel")) == 8
