"""The marshaller of caller-supplied rays (sampler._ray_args) and the rejections of its three callers, without a GPU and without
a context: every ValueError text is the one Sampler.aov_rays, radiance and radiance_adaptive raised before they shared it, and
the numpy path hands the caller's own arrays through.  Shapes: a 3 x 2 grid (nw = 3, nh = 2) and 5 rays."""
import numpy as np
import pytest
import torch

from micro_raytracer_amd import Sampler
from micro_raytracer_amd.sampler import _ray_args

f32 = np.float32
GRID = (2, 3, 3)
BOTH = "{fn}: orig and dir are both tensors on the context's device, or both host arrays"
ALL3 = "radiance: orig, dir and key are all tensors on the context's device, or all host arrays"
FREE = "radiance: orig and dir are [..., 3]"


def z(*shape):
    return np.zeros(shape, f32)


# (caller, orig, dir, required shape, key, the caller's text for mixed inputs, the text raised)
REJECTED = [(fn, *rest) for fn in ("aov_rays", "radiance_adaptive") for rest in (
    (z(2, 3, 3), z(3, 2, 3), GRID, None, None, f"{fn}: orig and dir are (2, 3, 3), got (2, 3, 3) and (3, 2, 3)"),        # mismatched shapes
    (z(3, 2, 3), z(3, 2, 3), GRID, None, None, f"{fn}: orig and dir are (2, 3, 3), got (3, 2, 3) and (3, 2, 3)"),        # the wrong grid
    (z(2, 3, 4), z(2, 3, 4), GRID, None, None, f"{fn}: orig and dir are (2, 3, 3), got (2, 3, 4) and (2, 3, 4)"),        # last axis not 3
    (z(2, 3, 3), None, GRID, None, None, f"{fn}: orig and dir are (2, 3, 3), got (2, 3, 3) and (1,)"),                   # orig without dir: None becomes array([nan])
    (torch.zeros(GRID), torch.zeros(GRID), GRID, None, None, BOTH.format(fn=fn)),                                        # torch CPU tensors
    (torch.zeros(GRID), z(2, 3, 3), GRID, None, None, BOTH.format(fn=fn)),
) if not (fn == "aov_rays" and rest[1] is None)          # aov_rays refuses one array without the other itself (below)
] + [
    ("radiance", z(5, 3), z(4, 3), None, None, ALL3, FREE),                                                              # mismatched shapes
    ("radiance", z(5, 4), z(5, 4), None, None, ALL3, FREE),                                                              # last axis not 3
    ("radiance", z(5, 3), None, None, None, ALL3, FREE),                                                                 # orig without dir
    ("radiance", z(5, 3), z(5, 3), None, np.zeros(4, np.uint32), ALL3, "radiance: one key per ray"),                     # a key too short
    ("radiance", z(2, 3, 3), z(2, 3, 3), None, np.zeros(5, np.uint32), ALL3, "radiance: one key per ray"),
    ("radiance", torch.zeros(5, 3), torch.zeros(5, 3), None, None, ALL3, ALL3),                                          # torch CPU tensors
    ("radiance", torch.zeros(5, 3), z(5, 3), None, None, ALL3, ALL3),
]


@pytest.mark.parametrize("case", REJECTED, ids=[f"{i}-{c[0]}" for i, c in enumerate(REJECTED)])
def test_rejection_texts(case):
    fn, orig, dir, shape, key, mixed, text = case
    with pytest.raises(ValueError) as e:
        _ray_args(fn, orig, dir, shape, key, mixed)
    assert str(e.value) == text


def test_callers_supply_their_own_texts():
    """What the marshaller does not know: radiance's text for mixed inputs, aov_rays' for one array without the other"""
    s = Sampler()
    s._ensure = lambda render: None               # no context: every call below is refused before it would need one
    s.nh, s.nw = GRID[:2]
    with pytest.raises(ValueError) as e:
        s.radiance(None, torch.zeros(5, 3), torch.zeros(5, 3), 1)
    assert str(e.value) == ALL3
    with pytest.raises(ValueError) as e:
        s.radiance(None, z(5, 3), z(5, 3), 1, key=np.zeros(6, np.uint32))
    assert str(e.value) == "radiance: one key per ray"
    with pytest.raises(ValueError) as e:
        s.radiance_adaptive(None, z(3, 2, 3), z(3, 2, 3), 0.0, max_samples=32)
    assert str(e.value) == "radiance_adaptive: orig and dir are (2, 3, 3), got (3, 2, 3) and (3, 2, 3)"
    for orig, dir in ((z(2, 3, 3), None), (None, z(2, 3, 3))):
        with pytest.raises(ValueError) as e:
            s.aov_rays(None, orig, dir)
        assert str(e.value) == "aov_rays: orig and dir are both given, or both None"
    with pytest.raises(ValueError) as e:
        s.aov_rays(None, None, None, wrap_x=True)
    assert str(e.value) == "aov_rays: wrap_x without rays"


@pytest.mark.parametrize("shape,required", [(GRID, GRID), ((5, 3), None)])
def test_numpy_arrays_pass_through(shape, required):
    """A contiguous float32 array is not copied, and the pointers are the arrays' own"""
    o, d, key = z(*shape), z(*shape), np.arange(int(np.prod(shape[:-1])), dtype=np.uint32)
    keep, ptrs, dev = _ray_args("radiance", o, d, required)
    assert keep[0] is o and keep[1] is d and len(keep) == 2
    assert list(ptrs) == [o.ctypes.data, d.ctypes.data, None] and dev is False
    keep, ptrs, dev = _ray_args("radiance", o, d, required, key)
    assert keep[2] is key and list(ptrs) == [o.ctypes.data, d.ctypes.data, key.ctypes.data] and dev is False


def test_numpy_arrays_are_made_contiguous_f32():
    o = np.zeros((5, 6), np.float64)[:, ::2]
    keep, ptrs, dev = _ray_args("radiance", o, o.tolist(), None, list(range(5)))
    assert [a.dtype for a in keep] == [f32, f32, np.uint32] and all(a.flags.c_contiguous for a in keep)
    assert list(ptrs) == [a.ctypes.data for a in keep] and dev is False
