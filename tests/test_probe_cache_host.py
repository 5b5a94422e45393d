"""emu.build.shared: one compilation and one binding of a probe per process, the same library for every caller."""
from emu import build as B


def test_shared_builds_and_binds_once():
    """var_probe (0.4 s), under build arguments no other module uses, so that the test does not depend on what ran before it"""
    bound = []
    kw = dict(with_pack=False, pthread=False)
    n0 = B.BUILDS.count("var_probe")
    first = B.shared("var_probe", bound.append, **kw)
    again = B.shared("var_probe", bound.append, **kw)
    assert again is first
    assert bound == [first]
    assert B.BUILDS.count("var_probe") == n0 + 1
    assert hasattr(first, "dv_filter")
