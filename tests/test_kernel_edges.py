"""Paths of the kernel the main parity sets never reach: sample indices at the top of the u32 range (the last chunk below
2^32, the look-ahead's plane sets there), the segment counter of the per-call loop, and the 4-wide triangle-BVH walk when
its walk area overflows (the deep-level and 1024-thread kernels on varied mesh scenes).  Same bars as the main sets:
mean radiance within 1e-4 of the oracle, NaN positions equal, tone-mapped bytes equal."""
import numpy as np
import pytest

from conftest import make_holder
from micro_raytracer_amd._abi import F_BVH, F_COLD, F_DEEP, F_IDENT
from test_fuzz_scenes import _check, crowd_scene, mesh_fuzz_scene

TOP = 0xffffffff


def _top_scenes():
    from micro_raytracer_amd import scenes
    return {
        "cornell": scenes.cornell_box(res=(24, 16), sample=1),
        "sink": scenes.kitchen_sink(res=(32, 20), sample=1),
        "mesh400": scenes.mesh_scene(res=(24, 14), sample=1, n_tris=400),
        "crowd": crowd_scene(3),
    }


# (base, n): the last chunk below 2^32 ending exactly at count == 0xffffffff, a base on the last chunk boundary, one sample
# below the chunk boundary before it, and the middle of the range (sign bit of the index)
TOP_CASES = [(TOP - n, n) for n in (1, 6, 31)] + [(0xfffffff0, n) for n in (1, 6)] + [(0xffffffe0 - 1, n) for n in (1, 6, 31)] \
    + [(2 ** 31 - 3, n) for n in (1, 6, 31)]


def _oracle_at(oracle_mod, h, seed, base, n):
    o = oracle_mod.Oracle(h, seed=seed)
    o.set_accum(np.zeros((o.nh, o.nw, 3), np.float32), base)
    o.execute(n)
    ref, cnt = o.accum()
    assert cnt == base + n
    return o, ref


@pytest.mark.parametrize("name", ["cornell", "sink", "mesh400", "crowd"])
def test_sample_indices_at_the_top_of_the_range_on_x86(name, oracle_mod, emu_mod):
    """render_pixel's chunk end min((chunk + 1) * kChunk, s_stop) must not wrap for the last chunk below 2^32 (sample indices
    0xfffffff0 and up): a wrapped end traces every index up to 0xffffffff instead of the ones asked for."""
    desc = _top_scenes()[name]
    render, h = make_holder(desc)
    if name == "crowd":
        assert emu_mod.layout(h)["features"] & F_BVH, "the crowd scene must take the instance-BVH kernels"
    for base, n in TOP_CASES:
        o, ref = _oracle_at(oracle_mod, h, 11, base, n)
        got, _ = emu_mod.render(h, 11, n, sample_base=base)
        _check(got, ref, n)
        o.set_accum(got, base + n)
        ss, out = emu_mod.img(h, got, base + n)
        assert np.array_equal(ss, o.img_ss()) and np.array_equal(out, o.img()), (base, n)


def _gpu_top_batched(render, oracle_h, oracle_mod, base, n, flags=0):
    from micro_raytracer_amd import Sampler
    s = Sampler(seed=11, flags=flags).create(render)
    s.set_accum(np.zeros((s.nh, s.nw, 3), np.float32), base)
    s.execute(render, n_samples=n)
    got, cnt = s.accum()
    assert cnt == base + n
    o, ref = _oracle_at(oracle_mod, oracle_h, 11, base, n)
    _check(got, ref, n)
    o.set_accum(got, cnt)
    assert np.array_equal(s.img_ss(), o.img_ss()) and np.array_equal(s.img(), o.img()), (base, n)
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "sink", "mesh400", "crowd"])
def test_sample_indices_at_the_top_of_the_range_gpu(name, oracle_mod):
    """The same bases through mrt_set_accum + one batched mrt_execute; the small frames split the samples over several lanes
    per pixel (k_split > 1), so the chunks of one call end at both chunk-end sites of render_pixel."""
    render, h = make_holder(_top_scenes()[name])
    split = 0
    for base, n in TOP_CASES:
        s = _gpu_top_batched(render, h, oracle_mod, base, n)
        split = max(split, s.stats()["k_split"])
        s.close()
    assert split > 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "mesh400"])
def test_per_call_loop_up_to_the_last_sample_index_gpu(name, oracle_mod):
    """One-sample mrt_execute calls up to count == 0xffffffff: the look-ahead's plane sets must not reach past the last index
    (the calls near the top fall back to their own launch), every return holds the plain loop's bits, the end equals the
    oracle, and the call past the limit fails with MRT_ERR_LIMIT and changes nothing.  The same under MRT_FLAG_DEFER."""
    from micro_raytracer_amd import Sampler, _abi, _lib
    render, h = make_holder(_top_scenes()[name])
    n = 45
    base = TOP - n
    ctx = {f: Sampler(seed=11, flags=f).create(render) for f in (0, _abi.FLAG_NO_LOOKAHEAD, _abi.FLAG_DEFER)}
    for s in ctx.values():
        s.set_accum(np.zeros((s.nh, s.nw, 3), np.float32), base)
    plain, ahead, defer = ctx[_abi.FLAG_NO_LOOKAHEAD], ctx[0], ctx[_abi.FLAG_DEFER]
    for i in range(n):
        plain.execute(render)
        ahead.execute(render)
        defer.execute(render)
        a, ca = plain.accum()
        b, cb = ahead.accum()
        assert ca == cb == base + i + 1 and np.array_equal(a.view(np.uint32), b.view(np.uint32)), i
    o, ref = _oracle_at(oracle_mod, h, 11, base, n)
    for s in ctx.values():
        got, cnt = s.accum()
        assert cnt == TOP
        _check(got, ref, n)
        with pytest.raises(_lib.MrtError) as e:
            s.execute(render)
        assert e.value.code == _abi.MRT_ERR_LIMIT
        again, cnt = s.accum()
        assert cnt == TOP and np.array_equal(again.view(np.uint32), got.view(np.uint32))
    o.set_accum(ahead.accum()[0], TOP)
    assert np.array_equal(ahead.img(), o.img())
    for s in ctx.values():
        s.close()


@pytest.mark.gpu
def test_segment_counter_of_every_per_call_execute():
    """MRT_FLAG_COUNT_SEGMENTS on the per-call loop: every one-sample mrt_execute reports the segments of its own sample, the
    same count a context without look-ahead reports, from the third call on too (where look-ahead would start)."""
    from micro_raytracer_amd import Sampler, _abi, scenes
    render, _ = make_holder(scenes.cornell_box(res=(64, 48), sample=6))
    a = Sampler(seed=5, flags=_abi.FLAG_COUNT_SEGMENTS)
    b = Sampler(seed=5, flags=_abi.FLAG_COUNT_SEGMENTS | _abi.FLAG_NO_LOOKAHEAD)
    for i in range(6):
        a.execute(render)
        b.execute(render)
        sa, sb = a.stats()["segments"], b.stats()["segments"]
        assert 64 * 48 <= sa == sb <= 64 * 48 * 9, (i, sa, sb)
        ra, ca = a.accum()
        rb, cb = b.accum()
        assert ca == cb == i + 1 and np.array_equal(ra.view(np.uint32), rb.view(np.uint32)), i
    a.close(); b.close()


MESH_FUZZ_SEEDS = list(range(16))


def _same_bits(a, b):
    """NaN in the same places, every other value the same bits (NaN payloads are not part of the contract)."""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


@pytest.mark.parametrize("seed", MESH_FUZZ_SEEDS)
def test_deep_walk_and_walk_area_overflow_on_x86(seed, oracle_mod, emu_mod, monkeypatch):
    """The F_DEEP lane code (4-wide triangle-BVH walk, level-ordered table, the first deep_nodes nodes staged) on meshes of
    300-1500 triangles, with walk areas down to 4 entries: a walk that fills its area answers through the reference's walk
    (mesh_walk4 returns 2).  Every form renders the bits of the default lane code, within the oracle bars; at 4 entries the
    fallback must actually have run."""
    render, h = make_holder(mesh_fuzz_scene(seed))
    spp = render.rt.sample
    o = oracle_mod.Oracle(h, seed=seed)
    o.execute(spp)
    ref, _ = o.accum()
    base, _ = emu_mod.render(h, seed, spp)
    _check(base, ref, spp)
    n_nodes = emu_mod.layout(h)["n_tbvh_nodes"]
    assert n_nodes > 40
    overflows = {}
    for cap in (4, 5, 6, 16):
        monkeypatch.setenv("MRT_EMU_WALK_CAP", str(cap))
        emu_mod.walk_overflows()
        for hot in (1, 7, n_nodes):
            got, _ = emu_mod.render(h, seed, spp, deep_nodes=hot)
            assert _same_bits(got, base), (cap, hot)
        overflows[cap] = emu_mod.walk_overflows()
    assert overflows[4] > 0, overflows
    o.set_accum(base, spp)
    ss, out = emu_mod.img(h, base, spp)
    assert np.array_equal(ss, o.img_ss()) and np.array_equal(out, o.img())


def test_mesh_route_at_large_scales_and_far_positions(emu_mod, monkeypatch):
    """The triangle-BVH routes (binary in two-leaf rounds, binary through leaf queues of 1 and 8 entries, and 4-wide at walk
    areas of 4 and 16 entries) against the reference's octree walk on
    meshes scaled by 1e-3 .. 1e3 and placed up to 1e5 from the origin (the route is taken below 1e6; a mesh stays at most
    ~1e4 of its sizes away, where f32 positions still resolve it): the culling margins of
    mrt_trace.h must hold where the rounding of the exact tests is largest."""
    import ctypes as C
    import mesh_probe
    from micro_raytracer_amd._abi import build_desc
    from micro_raytracer_amd.scene import load_render
    L = emu_mod.lib()
    L.emu_mesh_probe.restype = C.c_int
    # (scale, position range, mesh kind of tests/mesh_probe.py): the small end with hits comes from the soups and the grid meshes,
    # whose triangles stay large enough for the reference's test
    cases = [(1e-3, 5.0, 0), (0.03, 100.0, 1), (1.0, 1e4, 2), (50.0, 1e5, 3), (1e3, 1e5, 4), (1e3, 0.0, 0),
             (1e-2, 1e3, 2), (1e-2, 100.0, 4), (1e-2, 1e3, 4)]
    for seed, (scale, far, kind) in enumerate(cases):
        rng = np.random.default_rng(100 + seed)
        tris = (mesh_probe.random_mesh(rng, kind) * np.float32(scale)).astype(np.float32)
        pos = [float(x) for x in rng.uniform(-far, far, 3)]
        desc = {"frame": {"res": [8, 8]}, "scene": {"renderer": [{"type": "mesh", "mesh": [[[float(c) for c in vv] for vv in t] for t in tris], "pos": pos}]}}
        h = build_desc(load_render(desc))
        o, d = mesh_probe.rays_for(rng, tris, 4000)
        o = np.ascontiguousarray(o + np.asarray(pos, np.float32))
        # (the leaf queue of the warm binary walk at one entry -- a round per leaf -- and at kLeafQueue of mrt_trace.h)
        for cap, queue in ((4, 1), (16, 8)):
            monkeypatch.setenv("MRT_EMU_WALK_CAP", str(cap))
            monkeypatch.setenv("MRT_EMU_LEAF_QUEUE", str(queue))
            out = np.zeros((len(o), 10), np.uint32)
            stats = (C.c_uint32 * 2)()
            bad = L.emu_mesh_probe(C.cast(h.ptr(), C.c_void_p), len(o), o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p),
                                   out.ctypes.data_as(C.c_void_p), stats)
            # (below ~1e-2 the reference's own triangle test rejects every hit: its determinant falls under E)
            assert bad == 0 and stats[1] == 1 and (stats[0] > 100 or scale < 1e-2), (seed, scale, far, cap, bad, list(stats))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", MESH_FUZZ_SEEDS[:6])
def test_deep_walk_and_walk_area_overflow_gpu(seed, oracle_mod, monkeypatch, capfd):
    """The deep-level kernels (MRT_DEEP_NODES: the first n triangle-BVH nodes staged) with walk areas of 4 and 6 entries, in
    the default workgroup and in 1024-thread workgroups, on the mesh fuzz scenes: the bits of the whole-scene kernels
    (MRT_COLD=0), within the oracle bars, the same image bytes; at 4 entries walks overflow into the reference's walk."""
    import re
    from micro_raytracer_amd import Sampler, _lib
    render, h = make_holder(mesh_fuzz_scene(seed))
    spp = render.rt.sample
    o = oracle_mod.Oracle(h, seed=seed)
    o.execute(spp)
    ref, _ = o.accum()
    for k in ("MRT_COLD", "MRT_DEEP_NODES", "MRT_WALK_CAP", "MRT_BLOCK_THREADS", "MRT_DEBUG_FALLBACKS", "MRT_SCENE_IN_L2"):
        monkeypatch.delenv(k, raising=False)
    # the whole-scene kernels: from LDS where the scene fits, through L2 where it does not (MRT_COLD=0 takes the deep level then)
    monkeypatch.setenv("MRT_COLD", "0")
    if _lib.plan_launch(h)["kernel_features"] & (F_COLD | F_DEEP):
        monkeypatch.setenv("MRT_SCENE_IN_L2", "1")
    s = Sampler(seed=seed)
    s.execute(render, n_samples=spp)
    base, _ = s.accum()
    assert s.stats()["kernel_features"] & (F_COLD | F_DEEP) == 0
    s.close()
    monkeypatch.delenv("MRT_COLD")
    monkeypatch.delenv("MRT_SCENE_IN_L2", raising=False)
    _check(base, ref, spp)
    o.set_accum(base, spp)
    img_ss, img = o.img_ss(), o.img()
    monkeypatch.setenv("MRT_DEBUG_FALLBACKS", "1")
    full = {4: 0, 6: 0}
    n_mesh = sum(1 for r in render.scene.renderer if r.kind == "mesh")
    for hot in (str(n_mesh), "40"):                      # (the deep level stages every mesh's root at least)
        for cap in (4, 6):
            for threads in (None, "1024"):
                monkeypatch.setenv("MRT_DEEP_NODES", hot)
                monkeypatch.setenv("MRT_WALK_CAP", str(cap))
                if threads:
                    monkeypatch.setenv("MRT_BLOCK_THREADS", threads)
                else:
                    monkeypatch.delenv("MRT_BLOCK_THREADS", raising=False)
                capfd.readouterr()
                s = Sampler(seed=seed)
                s.execute(render, n_samples=spp)
                got, _ = s.accum()
                st = s.stats()
                err = capfd.readouterr().err
                what = (hot, cap, threads, st["kernel_features"], st["block_threads"])
                assert st["kernel_features"] & (F_COLD | F_DEEP) == (F_COLD | F_DEEP), what
                if threads:
                    assert st["block_threads"] == int(threads), what
                assert _same_bits(got, base), what
                assert np.array_equal(s.img_ss(), img_ss) and np.array_equal(s.img(), img), what
                m = re.findall(r"walk area full (\d+)", err)
                assert m, err
                full[cap] += int(m[-1])
                s.close()
    assert full[4] > 0, full


def test_ident_kernels_share_the_transform_bit_for_bit(emu_mod):
    """F_IDENT kernels send every ray through instance 0's matrices (X0, mrt_trace.h trace).  For every scene the packer marks
    all_ident, every instance's rot_y * (look * v) must give the same bits as X0's for v in {+-0, +-0.5, +-inf, NaN}^3.  Identities
    whose zeros differ in sign (the loader's default dir next to an explicit [0, 0, -1, 0]) fail that on a few vectors, so such
    a scene must not be all_ident; one sign everywhere keeps the F_IDENT kernels (and the bench scenes keep them)."""
    from micro_raytracer_amd import _lib, load_render, scenes
    import edge_cases
    from test_fuzz_scenes import ident_scene
    ec = edge_cases.cases()
    named = {"instance_grid": scenes.instance_grid(res=(32, 18), sample=1, n=4), "cornell": scenes.cornell_box(res=(16, 16), sample=1),
             "default": scenes.default_scene(res=(32, 18), sample=1), "uniform": ec["ident_zero_signs_uniform"],
             "mixed": ec["ident_zero_signs_mixed"]}
    named.update({f"ident_{k}": ident_scene(k) for k in range(10)})
    verdict = {}
    for name, desc in named.items():
        _, h = make_holder(desc)
        all_ident, bad = emu_mod.ident_xf(h)
        verdict[name] = all_ident
        if all_ident:
            assert bad == 0, (name, bad)
        assert bool(_lib.plan_launch(load_render(desc))["kernel_features"] & F_IDENT) == all_ident, name
    # the mixed scene really has identities that differ on such vectors, and is kept off the F_IDENT kernels
    _, h = make_holder(ec["ident_zero_signs_mixed"])
    assert emu_mod.ident_xf(h)[1] > 0 and not verdict["mixed"]
    assert all(v for k, v in verdict.items() if k != "mixed"), verdict
