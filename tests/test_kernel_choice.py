"""Which build of the trace kernel a launch runs, without a GPU (include/hrt.h hrt_debug_pick_kernel; csrc/hrt_api.hip k_builds,
pick_build): the library's choice against an independent statement of the rule over the full product of its inputs' edges, the
wording of its refusals, the flags that must not matter, and the table of builds against the kernels the sources define.

The sources define 30 trace kernels: 10 lane-per-pixel, 4 two-stream, 16 workgroup-streaming."""
import ctypes as C
import glob
import itertools
import os
import re

import pytest

HRT_OK, HRT_ERR_INVALID = 0, -1
GAMMA, NO_LDS, WAVE, STREAM, NO_CULL, DUAL, EXACT, BRUTE = 1, 2, 4, 8, 16, 32, 64, 128
SPH_MIN = 8  # HRT_SPHERE_FILTER_MIN (csrc/hrt_kernels.hip)
N_BUILDS = 10 + 4 + 16
FORM_FLAGS = [sum(c) for r in range(6) for c in itertools.combinations((WAVE, STREAM, DUAL, EXACT, BRUTE), r)]
PRODUCT = dict(n_meshes=(0, 1), n_lights=(0, 1), n_spheres=(0, SPH_MIN - 1, SPH_MIN, 128, 129), tab_rows=(3072, 3073), tiles=(1, 5120, 5121),
               spp=(1, 7, 8), flags=FORM_FLAGS, has_list=(0, 1), n_views=(0, 3), kernel=("", "single", "dual", "stream"))


def expected(n_meshes, n_lights, n_spheres, tab_rows, tiles, spp, flags, has_list, n_views, kernel):
    """The rule, restated: a kernel name, or None where the launch is refused."""
    use_dual, use_stream = kernel != "single", {"stream": 1, "single": 0, "dual": 0}.get(kernel, -1)
    fits = tab_rows * 16 <= 48 * 1024
    exact = bool(flags & EXACT)
    if ((flags & STREAM) and not fits) or ((flags & BRUTE) and not exact) or (exact and (flags & DUAL)):
        return None
    pays = n_meshes > 0 or n_lights > 0 or (tiles <= 5120 and spp >= 8)
    stream = fits and not flags & (WAVE | DUAL) and (use_stream == 1 or bool(flags & STREAM) or (use_stream < 0 and pays))
    dual = not exact and not stream and not n_views and (use_dual or bool(flags & DUAL)) and n_meshes > 0 and not flags & WAVE
    if n_views and (has_list or exact):
        return None  # no such builds
    sph = stream and not exact and SPH_MIN <= n_spheres <= 128
    return ("hrt_wgstream_kernel" if stream else "hrt_trace2_kernel" if dual else "hrt_trace_kernel") + ("_lights" if n_lights else "") + \
        ("_sph" if sph else "_exact" if exact else "") + ("_list" if has_list else "_views" if n_views else "")


def make_picker(hrt):
    dev = hrt.device_lib()
    name, inp = C.create_string_buffer(64), hrt.PickInput()
    call, ref = dev.hrt_debug_pick_kernel, C.byref(inp)

    def pick(n_meshes, n_lights, n_spheres, tab_rows, tiles, spp, flags, has_list, n_views, kernel):
        inp.n_meshes, inp.n_lights, inp.n_spheres, inp.tab_rows, inp.tiles, inp.spp = n_meshes, n_lights, n_spheres, tab_rows, tiles, spp
        inp.flags, inp.has_list, inp.n_views, inp.hrt_kernel = flags, has_list, n_views, kernel.encode()
        return call(ref, name, 64), name.value.decode()
    return pick


@pytest.fixture(scope="module")
def reached(hrt):
    """The library's answer over the whole product, checked against the restated rule on the way: the set of names it gave."""
    pick, names = make_picker(hrt), set()
    for case in itertools.product(*PRODUCT.values()):
        rc, got = pick(*case)
        want = expected(*case)
        assert (rc, got) == ((HRT_OK, want) if want else (HRT_ERR_INVALID, "")), (dict(zip(PRODUCT, case)), rc, got, want)
        names.add(got)
    return names - {""}


def test_the_choice_is_the_restated_rule_over_the_full_product(reached):
    assert reached


def defined_kernels():
    """The trace kernels the sources define: extern "C" __global__ functions of a const DRender R, by their family's prefix."""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hai719-raytracing_amd", "csrc", "*.hip")
    pattern = r'extern "C" __global__ void (?:__launch_bounds__\([^)]*\) )?((?:hrt_trace_kernel|hrt_trace2_kernel|hrt_wgstream_kernel)\w*)\(const DRender R\)'
    return {name for path in glob.glob(src) for name in re.findall(pattern, open(path).read())}


def test_the_table_and_the_sources_agree(reached):
    """A kernel defined without a row is never named; a row nobody can reach is never named either."""
    defined = defined_kernels()
    assert reached == defined, (sorted(defined - reached), sorted(reached - defined))
    assert len(reached) == N_BUILDS


def test_pick_kernel_wrapper_names_or_raises(hrt):
    assert hrt.pick_kernel(1, 1, 0, 100, 6, 2) == "hrt_wgstream_kernel_lights"
    assert hrt.pick_kernel(1, 0, 0, 100, 6, 2, has_list=True, kernel="dual") == "hrt_trace2_kernel_list"
    assert hrt.pick_kernel(1, 0, 0, 100, 6, 2, n_views=3, kernel="dual") == "hrt_trace_kernel_views"  # the preference yields to views
    with pytest.raises(hrt.HrtError, match="batched views"):
        hrt.pick_kernel(0, 0, 0, 100, 6, 2, flags=EXACT, n_views=3)


@pytest.mark.parametrize("flags,tab_rows,words", [
    (STREAM, 3073, "the scene's object tables exceed the 48 KiB the streaming kernel keeps in LDS; use another kernel form"),
    (BRUTE, 3072, "flags: HRT_FLAG_MESH_BRUTE needs HRT_FLAG_EXACT_ONLY"),
    (EXACT | DUAL, 3072, "no exact-only build of the two-stream kernel")])
def test_refusals_keep_their_wording(hrt, flags, tab_rows, words):
    rc, name = make_picker(hrt)(1, 1, 8, tab_rows, 6, 2, flags, 0, 0, "")
    msg = hrt.device_lib().hrt_last_error().decode()
    assert rc == HRT_ERR_INVALID and name == "" and msg.startswith("render: ") and words in msg, msg


def test_refusals_come_in_the_stated_order(hrt):
    pick, err = make_picker(hrt), hrt.device_lib().hrt_last_error
    assert pick(1, 1, 8, 3073, 6, 2, STREAM | BRUTE | DUAL, 0, 0, "")[0] == HRT_ERR_INVALID and b"48 KiB" in err()
    assert pick(1, 1, 8, 3072, 6, 2, STREAM | BRUTE | DUAL, 0, 0, "")[0] == HRT_ERR_INVALID and b"MESH_BRUTE" in err()
    assert pick(1, 1, 8, 3072, 6, 2, STREAM | BRUTE | DUAL | EXACT, 0, 0, "")[0] == HRT_ERR_INVALID and b"two-stream" in err()


@pytest.mark.parametrize("inert", [GAMMA, NO_LDS, NO_CULL])
def test_inert_flags_never_change_the_answer(hrt, inert):
    pick = make_picker(hrt)
    keys = list(PRODUCT)
    for case in itertools.product(*PRODUCT.values()):
        with_inert = list(case)
        with_inert[keys.index("flags")] |= inert
        assert pick(*with_inert) == pick(*case), dict(zip(keys, case))


def test_null_arguments_are_refused(hrt):
    dev = hrt.device_lib()
    name = C.create_string_buffer(8)
    assert dev.hrt_debug_pick_kernel(None, name, 8) == HRT_ERR_INVALID
    assert dev.hrt_debug_pick_kernel(C.byref(hrt.PickInput()), None, 8) == HRT_ERR_INVALID
    assert dev.hrt_debug_last_kernel(None, name, 8) == HRT_ERR_INVALID
    assert dev.hrt_debug_pick_kernel(C.byref(hrt.PickInput(spp=1, tiles=1)), name, 8) == HRT_OK and name.value == b"hrt_tra"  # cut to cap
