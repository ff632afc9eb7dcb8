"""ctypes bindings over the two C-ABI libraries of the MI355X ray-trace path.

* ``libhrt_host.so`` -- host scene layer (``include/hrt_host.h``): Scene / Mesh /
  Material set-up with the reference's interface, flattened KD-tree builder.
* ``libhrt.so``      -- HIP kernels for gfx950 behind ``include/hrt.h``; the drop-in
  for the reference's ``ray_trace_from_camera()`` (/root/reference/main.cpp:200-263).

There is NO CPU fallback: if ``libhrt.so`` is missing or no GPU is present every
render entry point raises.  The package directory name contains a hyphen, so
import it with ``importlib.import_module("hai719-raytracing_amd")``.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
REPO_ROOT = os.path.dirname(_HERE)
ASSET_ROOT = os.path.join(REPO_ROOT, "assets")
TILE = 8  # HRT_TILE

FLAG_GAMMA = 1
FLAG_NO_LDS_TREE = 2
FLAG_WAVE_KERNEL = 4
FLAG_STREAM_KERNEL = 8
FLAG_NO_SHADOW_CULL = 16
FLAG_DUAL_KERNEL = 32
FLAG_EXACT_ONLY = 64   # proof builds: no filters, no reciprocal approximations (include/hrt.h)
FLAG_MESH_BRUTE = 128  # with FLAG_EXACT_ONLY: every triangle of a gated mesh, no KD walk

MAT_DIFFUSE, MAT_GLASS, MAT_MIRROR = 0, 1, 2
TEX_NONE, TEX_CHECKER, TEX_IMAGE = 0, 1, 2


class HrtError(RuntimeError):
    pass


class SceneDescPtr(C.c_void_p):
    """``const hrt_scene_desc*`` that keeps the HostScene owning the memory alive."""


# ----------------------------------------------------------------- PODs (hrt.h)
class Material(C.Structure):
    _fields_ = [
        ("albedo", C.c_float * 3), ("transparency", C.c_float), ("index_medium", C.c_float),
        ("type", C.c_int32), ("texture_type", C.c_int32),
        ("checker1", C.c_float * 3), ("checker2", C.c_float * 3),
        ("tex_scale_x", C.c_float), ("tex_scale_y", C.c_float),
        ("emissive", C.c_int32), ("light_color", C.c_float * 3), ("light_intensity", C.c_float),
        ("image", C.c_int32), ("normal_map", C.c_int32), ("motion", C.c_float * 3),
    ]

    @staticmethod
    def make(albedo=(0.8, 0.8, 0.8), type=MAT_DIFFUSE, transparency=0.0, index_medium=1.0,
             emissive=False, light_color=(0, 0, 0), light_intensity=0.0, motion=(0, 0, 0),
             texture_type=TEX_NONE, image=-1, normal_map=-1, checker1=(0, 0, 0), checker2=(0, 0, 0),
             tex_scale=(1.0, 1.0)) -> "Material":
        m = Material()
        m.albedo[:] = albedo
        m.type = type
        m.transparency = transparency
        m.index_medium = index_medium
        m.emissive = int(bool(emissive))
        m.light_color[:] = light_color
        m.light_intensity = light_intensity
        m.motion[:] = motion
        m.texture_type = texture_type
        m.image = image
        m.normal_map = normal_map
        m.checker1[:] = checker1
        m.checker2[:] = checker2
        m.tex_scale_x, m.tex_scale_y = tex_scale
        return m


class Camera(C.Structure):
    _fields_ = [
        ("eye", C.c_float * 3), ("right", C.c_float * 3), ("up", C.c_float * 3), ("forward", C.c_float * 3),
        ("fovy_deg", C.c_float), ("aspect", C.c_float), ("znear", C.c_float), ("zfar", C.c_float),
    ]


class View(C.Structure):
    """``hrt_view``: one camera of a batched render with the seed of its frame (include/hrt.h)."""
    _fields_ = [("cam", Camera), ("seed", C.c_uint64)]


LENS_PERSPECTIVE, LENS_ORTHOGRAPHIC, LENS_EQUIRECT, LENS_FISHEYE = 0, 1, 2, 3
LENS_DRAW = 0x80000000  # HRT_LENS_DRAW: draw index of the first of the two lens draws
_PROJECTIONS = {"perspective": LENS_PERSPECTIVE, "ortho": LENS_ORTHOGRAPHIC, "orthographic": LENS_ORTHOGRAPHIC,
                "equirect": LENS_EQUIRECT, "fisheye": LENS_FISHEYE}


class Lens(C.Structure):
    """``hrt_lens``: a camera with a projection (include/hrt.h "Lens cameras").  ``projection``: "perspective", "ortho", "equirect",
    "fisheye" or a LENS_* value; ``aperture`` and ``focus``: the thin lens' radius and the depth along forward of the plane in focus
    (perspective only); ``extent``: the height of the view volume (ortho) or the field of view in degrees (fisheye)."""
    _fields_ = [("cam", Camera), ("projection", C.c_uint32), ("aperture_radius", C.c_float), ("focus_distance", C.c_float),
                ("extent", C.c_float)]

    def __init__(self, cam: Camera, projection="perspective", aperture: float = 0.0, focus: float = 1.0, extent: float = 0.0):
        super().__init__()
        if isinstance(projection, str):
            if projection not in _PROJECTIONS:
                raise ValueError(f"Lens: projection must be one of {sorted(_PROJECTIONS)} (got {projection!r})")
            projection = _PROJECTIONS[projection]
        self.cam = cam
        self.projection = int(projection)
        self.aperture_radius = aperture
        self.focus_distance = focus
        self.extent = extent


class LensView(C.Structure):
    """``hrt_lens_view``: one lens camera of a batched lens render with the seed of its frame (include/hrt.h)."""
    _fields_ = [("lens", Lens), ("seed", C.c_uint64)]


class Quad(C.Structure):
    """``hrt_quad``: a square of a flattened scene (include/hrt.h) -- corner v0, its neighbours v1 and v3, the normal-map frame."""
    _fields_ = [("v0", C.c_float * 3), ("v1", C.c_float * 3), ("v3", C.c_float * 3), ("tangent", C.c_float * 3),
                ("bitangent", C.c_float * 3), ("material", C.c_int32)]

    @staticmethod
    def make(v0, v1, v3, material: int = 0) -> "Quad":
        q = Quad()
        q.v0[:], q.v1[:], q.v3[:] = v0, v1, v3
        q.material = material
        return q


class PickInput(C.Structure):
    """hrt_pick_input (include/hrt.h): what the choice of a trace kernel build depends on."""
    _fields_ = [("n_meshes", C.c_uint32), ("n_lights", C.c_uint32), ("n_spheres", C.c_uint32), ("tab_rows", C.c_uint32),
                ("tiles", C.c_uint32), ("spp", C.c_uint32), ("flags", C.c_uint32), ("has_list", C.c_uint32), ("n_views", C.c_uint32),
                ("hrt_kernel", C.c_char_p)]


class Stats(C.Structure):
    _fields_ = [
        ("kernel_ms", C.c_double), ("total_ms", C.c_double), ("samples", C.c_uint64),
        ("vgprs", C.c_uint32), ("sgprs", C.c_uint32), ("lds_bytes", C.c_uint32), ("waves_launched", C.c_uint32),
    ]


class Adaptive(C.Structure):
    """``hrt_adaptive``: parameters of adaptive sampling (include/hrt.h)."""
    _fields_ = [("min_spp", C.c_uint32), ("max_spp", C.c_uint32), ("threshold", C.c_float)]


FEATURE_FLOATS = 12  # HRT_FEATURE_FLOATS: albedo rgb, normal xyz, emission rgb, depth, coverage, 0


# Ray queries (include/hrt.h hrt_trace_rays).  A ray is RAY_FLOATS float32: origin, time, direction, tmax.
RAY_FLOATS = 8
RAY_O, RAY_TIME, RAY_D, RAY_TMAX = slice(0, 3), 3, slice(4, 7), 7
QUERY_CLOSEST, QUERY_SHADE, QUERY_OCCLUDED = 0, 1, 2
RAYS_NORMALIZE = 256  # HRT_RAYS_NORMALIZE: the Ray constructor's normalisation of d first
_QUERY_MODES = {"closest": QUERY_CLOSEST, "shade": QUERY_SHADE, "occluded": QUERY_OCCLUDED}
# Columns of a CLOSEST / SHADE record.  Records come back as float32; the integer columns (kind, index, prim, material type) hold
# u32 bits: read them with .view(np.uint32) (numpy) or .view(torch.int32) (torch).
HIT_T, HIT_KIND, HIT_INDEX, HIT_PRIM = 0, 1, 2, 3
CLOSEST_FLOATS = 4
SHADE_NORMAL, SHADE_TRANSPARENCY = slice(4, 7), 7
SHADE_ALBEDO, SHADE_INDEX_MEDIUM = slice(8, 11), 11
SHADE_EMISSION, SHADE_MATERIAL_TYPE = slice(12, 15), 15
SHADE_FLOATS = 16
KIND_MISS, KIND_SPHERE, KIND_SQUARE, KIND_MESH = 0, 1, 2, 3
NO_PRIM = 0xFFFFFFFF  # index and prim of a miss, prim of a sphere or square hit
RADIANCE_ACCUMULATE = 512  # HRT_RADIANCE_ACCUMULATE: add to the running sums in the output instead of storing means
# Light probes (include/hrt.h "Light probes").  A probe record is PROBE_FLOATS float32: position, time; a result PROBE_COEFFS x 3.
PROBE_FLOATS = 4    # HRT_PROBE_FLOATS
PROBE_COEFFS = 9    # HRT_PROBE_COEFFS
PROBE_BLOCK = 64    # HRT_PROBE_BLOCK: samples per block of the fixed-order sum (tests/test_probe_abi.py holds it to the header)
PROBE_RECORD_FLOATS = 32      # HRT_PROBE_RECORD_FLOATS: a probe's packed record inside a ProbeVolume, 27 coefficients + 5 zeros
PROBE_VOLUME_MAX = 1 << 24    # HRT_PROBE_VOLUME_MAX: probes per volume
PROBE_EVAL_RADIANCE = 1       # HRT_PROBE_EVAL_RADIANCE: SH radiance in direction N instead of the cosine-convolved irradiance / pi
PROBE_EVAL_FACING = 2         # HRT_PROBE_EVAL_FACING: weight probes by how far they face the surface
PROBE_DEPTH_RES = 8                 # HRT_PROBE_DEPTH_RES: a probe's octahedral depth map is RES x RES texels
PROBE_DEPTH_TEXELS = 64             # HRT_PROBE_DEPTH_TEXELS
PROBE_DEPTH_FLOATS = 192            # HRT_PROBE_DEPTH_FLOATS: the sums {W, A, B} per texel
PROBE_DEPTH_MAX_BLOCKS = 1 << 20    # HRT_PROBE_DEPTH_MAX_BLOCKS: (probe, block of 64 samples) pairs per depth launch
PROBE_DEPTH_VOLUME_MAX = 1 << 22    # HRT_PROBE_DEPTH_VOLUME_MAX: probes of a volume with depth
LIT_VISIBLE = 4                     # HRT_LIT_VISIBLE: eval_flags of trace_lit / probes_lit: the look-up of "Probe visibility"
# Lit paths (include/hrt.h "Lit paths").  A tail record is TAIL_FLOATS float32: {p, time, n, bias}, thr, the word, rad / 6, 0.
TAIL_FLOATS = 16                    # HRT_TAIL_FLOATS
TAIL_WORD = 11                      # the column of the uint32 word: bits 0..7 the segments traced, TAIL_REACHED
TAIL_REACHED = 0x80000000           # HRT_TAIL_REACHED
MAXBOUNCES = 6                      # HRT_MAXBOUNCES: the largest tail_after
GUIDES_FIRST_HIT = 0                # HRT_GUIDES_FIRST_HIT: denoiser guides from render_features
GUIDES_FIRST_DIFFUSE = 1            # HRT_GUIDES_FIRST_DIFFUSE: denoiser guides from render_path_features ("Path features")
_GUIDES = {"first": GUIDES_FIRST_HIT, "diffuse": GUIDES_FIRST_DIFFUSE}


def _guides_arg(who: str, guides) -> int:
    """The ``guides`` keyword of the guided renders: "first" or "diffuse" -> HRT_GUIDES_*."""
    if guides not in _GUIDES:
        raise ValueError(f"{who}: guides must be \"first\" or \"diffuse\" (got {guides!r})")
    return _GUIDES[guides]


class DenoiseParams(C.Structure):
    """``hrt_denoise_params``: the a-trous filter's iteration count and edge-stopping widths (include/hrt.h).  The defaults were
    chosen by tools/denoise_report.py's sweep ("Denoising")."""
    _fields_ = [("iterations", C.c_uint32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_albedo", C.c_float),
                ("sigma_depth", C.c_float)]

    def __init__(self, iterations=4, sigma_color=8.0, sigma_normal=0.05, sigma_albedo=0.4, sigma_depth=0.05):
        super().__init__(iterations, sigma_color, sigma_normal, sigma_albedo, sigma_depth)


class DenoiseVarParams(C.Structure):
    """``hrt_denoise_var_params``: the variance-guided filter's iteration and prefilter counts, the colour width in standard
    deviations of the difference of a pair of pixels' own means, the guide widths and the variance floor (include/hrt.h).  The defaults were chosen by
    tools/denoise_report.py --var ("Variance-guided denoising")."""
    _fields_ = [("iterations", C.c_uint32), ("prefilter", C.c_uint32), ("sigma_variance", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_albedo", C.c_float), ("sigma_depth", C.c_float), ("variance_floor", C.c_float)]

    def __init__(self, iterations=4, prefilter=2, sigma_variance=8.0, sigma_normal=0.05, sigma_albedo=0.4, sigma_depth=0.05,
                 variance_floor=1e-8):
        super().__init__(iterations, prefilter, sigma_variance, sigma_normal, sigma_albedo, sigma_depth, variance_floor)


class TemporalParams(C.Structure):
    """``hrt_temporal_params``: the floor of the current frame's blend weight, the history length at which accumulation saturates,
    and what a reprojected tap may differ by in relative depth, |normal difference|^2 and |albedo difference|^2 (include/hrt.h)."""
    _fields_ = [("alpha_min", C.c_float), ("max_history", C.c_float), ("depth_tol", C.c_float), ("normal_tol", C.c_float),
                ("albedo_tol", C.c_float)]

    def __init__(self, alpha_min=0.02, max_history=64.0, depth_tol=0.05, normal_tol=0.1, albedo_tol=0.05):
        super().__init__(alpha_min, max_history, depth_tol, normal_tol, albedo_tol)


def _load(name: str) -> C.CDLL:
    path = os.path.join(_HERE, name)
    if not os.path.exists(path):
        raise HrtError(f"{path} is missing: run `python __graft_entry__.py` (build()) or `make -C {_HERE}` first")
    return C.CDLL(path, mode=C.RTLD_GLOBAL)


_host: Optional[C.CDLL] = None
_dev: Optional[C.CDLL] = None


def host_lib() -> C.CDLL:
    global _host
    if _host is None:
        lib = _load("libhrt_host.so")
        lib.hrt_host_last_error.restype = C.c_char_p
        lib.hrt_host_scene_new.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        lib.hrt_host_scene_free.argtypes = [C.c_void_p]
        lib.hrt_host_scene_free.restype = None
        lib.hrt_host_scene_setup.argtypes = [C.c_void_p, C.c_char_p, C.c_float, C.c_uint64]
        lib.hrt_host_scene_clear.argtypes = [C.c_void_p]
        lib.hrt_host_scene_add_texture.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
        lib.hrt_host_scene_add_normal_map.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
        lib.hrt_host_scene_set_skybox.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
        lib.hrt_host_scene_add_sphere.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_float, C.POINTER(Material)]
        lib.hrt_host_scene_add_quad.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                                C.POINTER(C.c_float), C.c_float, C.c_float, C.POINTER(Material)]
        lib.hrt_host_scene_add_mesh.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                                C.c_void_p, C.POINTER(Material)]
        lib.hrt_host_scene_add_mesh_off.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(Material)]
        lib.hrt_host_scene_add_light.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_float, C.POINTER(C.c_float)]
        lib.hrt_host_scene_set_sky.argtypes = [C.c_void_p, C.c_int32]
        lib.hrt_host_scene_set_kd_params.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        lib.hrt_host_scene_set_kd_builder.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.hrt_host_scene_flatten.argtypes = [C.c_void_p, C.c_void_p]
        lib.hrt_host_scene_kd_stats.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        lib.hrt_host_scene_irregular_stats.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        lib.hrt_host_default_camera.argtypes = [C.c_float, C.POINTER(Camera)]
        lib.hrt_host_default_camera.restype = None
        _host = lib
    return _host


def device_lib() -> C.CDLL:
    """The HIP library.  Raises if it has not been built -- there is no fallback."""
    global _dev
    if _dev is None:
        lib = _load(os.environ.get("HRT_LIBNAME", "libhrt.so"))  # HRT_LIBNAME: A/B builds of the same ABI (tools/variants.sh)
        lib.hrt_last_error.restype = C.c_char_p
        lib.hrt_init.argtypes = [C.c_int]
        lib.hrt_shutdown.restype = None
        lib.hrt_scene_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        lib.hrt_scene_destroy.argtypes = [C.c_void_p]
        lib.hrt_scene_destroy.restype = None
        lib.hrt_render.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                   C.c_uint32, C.c_void_p, C.POINTER(Stats)]
        lib.hrt_tiles_total.argtypes = [C.c_uint32, C.c_uint32]
        lib.hrt_tiles_total.restype = C.c_uint32
        lib.hrt_tiles_owned.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
        lib.hrt_tiles_owned.restype = C.c_uint32
        lib.hrt_render_tiles.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                         C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.hrt_assemble_frame.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                           C.c_void_p]
        lib.hrt_last_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        lib.hrt_check_last_launch.argtypes = [C.c_void_p]
        lib.hrt_kernel_info.argtypes = [C.POINTER(Stats)]
        lib.hrt_write_ppm.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint32]
        lib.hrt_render_accumulate.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                              C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.hrt_finalize_tiles.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.hrt_encode_ppm.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t,
                                       C.POINTER(C.c_size_t), C.c_void_p]
        lib.hrt_multi_create.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_int), C.POINTER(C.c_void_p)]
        lib.hrt_multi_render.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                         C.c_uint32, C.c_void_p, C.POINTER(Stats)]
        lib.hrt_multi_destroy.argtypes = [C.c_void_p]
        lib.hrt_multi_destroy.restype = None
        lib.hrt_multi_gather.argtypes = [C.c_void_p]
        lib.hrt_multi_gather.restype = C.c_char_p
        lib.hrt_render_multi.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                         C.c_uint32, C.c_uint32, C.POINTER(C.c_int), C.c_void_p, C.POINTER(Stats)]
        lib.hrt_render_adaptive.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.POINTER(Adaptive), C.c_uint64,
                                            C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        lib.hrt_render_adaptive_tiles.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.POINTER(Adaptive),
                                                  C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.hrt_render_features.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                            C.c_void_p, C.c_void_p]
        lib.hrt_denoise_scratch_bytes.argtypes = [C.c_uint32, C.c_uint32]
        lib.hrt_denoise_scratch_bytes.restype = C.c_size_t
        lib.hrt_denoise.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(DenoiseParams), C.c_uint32, C.c_void_p,
                                    C.c_void_p, C.c_void_p]
        lib.hrt_render_denoised.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                            C.c_uint32, C.POINTER(DenoiseParams), C.c_void_p, C.POINTER(Stats)]
        lib.hrt_denoise_var_scratch_bytes.argtypes = [C.c_uint32, C.c_uint32]
        lib.hrt_denoise_var_scratch_bytes.restype = C.c_size_t
        lib.hrt_denoise_var.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(DenoiseVarParams), C.c_uint32,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.hrt_render_denoised_var.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                                C.c_uint32, C.POINTER(DenoiseVarParams), C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        lib.hrt_temporal_accumulate.argtypes = [C.POINTER(Camera), C.POINTER(Camera), C.c_uint32, C.c_uint32] + [C.c_void_p] * 7 + \
                                              [C.POINTER(TemporalParams)] + [C.c_void_p] * 4
        lib.hrt_history_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        lib.hrt_history_reset.argtypes = [C.c_void_p]
        lib.hrt_history_reset.restype = None
        lib.hrt_history_destroy.argtypes = [C.c_void_p]
        lib.hrt_history_destroy.restype = None
        lib.hrt_render_temporal.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                            C.c_uint64, C.c_uint32, C.POINTER(TemporalParams), C.POINTER(DenoiseVarParams), C.c_void_p,
                                            C.c_void_p, C.POINTER(Stats)]
        lib.hrt_debug_kat.argtypes = [C.c_uint32, C.POINTER(Camera), C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        lib.hrt_trace_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.hrt_trace_radiance.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                           C.c_uint32, C.c_void_p, C.c_void_p]
        lib.hrt_camera_rays.argtypes = [C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p]
        lib.hrt_render_views_device.argtypes = [C.c_void_p, C.POINTER(View), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                C.c_void_p, C.c_void_p]
        lib.hrt_render_views.argtypes = [C.c_void_p, C.POINTER(View), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.c_void_p, C.POINTER(Stats)]
        lib.hrt_lens_rays.argtypes = [C.POINTER(Lens), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p]
        lib.hrt_render_lens_device.argtypes = [C.c_void_p, C.POINTER(Lens), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                               C.c_uint32, C.c_void_p, C.c_void_p]
        lib.hrt_render_lens.argtypes = [C.c_void_p, C.POINTER(Lens), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32,
                                        C.c_void_p, C.POINTER(Stats)]
        lib.hrt_render_lens_adaptive_device.argtypes = [C.c_void_p, C.POINTER(Lens), C.c_uint32, C.c_uint32, C.POINTER(Adaptive), C.c_uint64,
                                                        C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.hrt_render_lens_adaptive.argtypes = [C.c_void_p, C.POINTER(Lens), C.c_uint32, C.c_uint32, C.POINTER(Adaptive), C.c_uint64,
                                                 C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        lib.hrt_render_lens_features.argtypes = [C.c_void_p, C.POINTER(Lens), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                                 C.c_void_p, C.c_void_p]
        lib.hrt_render_lens_views_device.argtypes = [C.c_void_p, C.POINTER(LensView), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                     C.c_uint32, C.c_void_p, C.c_void_p]
        lib.hrt_render_lens_views.argtypes = [C.c_void_p, C.POINTER(LensView), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                              C.c_void_p, C.POINTER(Stats)]
        lib.hrt_render_lens_views_features.argtypes = [C.c_void_p, C.POINTER(LensView), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                       C.c_void_p, C.c_void_p]
        lib.hrt_bake_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p]
        lib.hrt_bake_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32,
                                        C.c_void_p, C.c_void_p]
        lib.hrt_bake.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p,
                                 C.POINTER(Stats)]
        lib.hrt_bake_quad_points.argtypes = [C.POINTER(Quad), C.c_uint32, C.c_uint32, C.c_int32, C.c_float, C.c_float, C.c_void_p]
        lib.hrt_bake_mesh_points.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_void_p]
        lib.hrt_probe_rays.argtypes = lib.hrt_bake_rays.argtypes
        lib.hrt_probes_device.argtypes = lib.hrt_bake_device.argtypes
        lib.hrt_probes.argtypes = lib.hrt_bake.argtypes
        lib.hrt_probe_grid_points.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p]
        lib.hrt_probe_volume_create.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
        lib.hrt_probe_volume_update_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.hrt_probe_volume_update.argtypes = [C.c_void_p, C.c_void_p]
        lib.hrt_probe_volume_destroy.argtypes = [C.c_void_p]
        lib.hrt_probe_volume_destroy.restype = None
        lib.hrt_probe_eval_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.hrt_probe_eval.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(Stats)]
        lib.hrt_probe_volume_weights.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                                 C.c_void_p]
        lib.hrt_probe_depth_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_float,
                                               C.c_uint32, C.c_void_p, C.c_void_p]
        lib.hrt_probe_depth.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_float, C.c_uint32, C.c_void_p,
                                        C.POINTER(Stats)]
        lib.hrt_probe_volume_update_depth_device.argtypes = lib.hrt_probe_volume_update_device.argtypes
        lib.hrt_probe_volume_update_depth.argtypes = lib.hrt_probe_volume_update.argtypes
        lib.hrt_probe_eval_visible_device.argtypes = lib.hrt_probe_eval_device.argtypes
        lib.hrt_probe_eval_visible.argtypes = lib.hrt_probe_eval.argtypes
        lib.hrt_probe_depth_texel.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        lib.hrt_probe_depth_direction.argtypes = [C.c_uint32, C.c_void_p]
        lib.hrt_trace_lit.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32,
                                      C.c_uint32, C.c_float, C.c_void_p, C.c_void_p]
        lib.hrt_probes_lit_device.argtypes = lib.hrt_trace_lit.argtypes
        lib.hrt_probes_lit.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32,
                                       C.c_float, C.c_void_p, C.POINTER(Stats)]
        lib.hrt_trace_lit_paths.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32,
                                            C.c_uint32, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.hrt_probes_lit_paths_device.argtypes = lib.hrt_trace_lit_paths.argtypes
        lib.hrt_probes_lit_paths.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32,
                                             C.c_float, C.c_uint32, C.c_void_p, C.POINTER(Stats)]
        lib.hrt_path_tails.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_float, C.c_uint32,
                                       C.c_void_p, C.c_void_p]
        lib.hrt_path_features.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.hrt_render_path_features.argtypes = lib.hrt_render_features.argtypes
        lib.hrt_render_lens_path_features.argtypes = lib.hrt_render_lens_features.argtypes
        lib.hrt_render_lens_views_path_features.argtypes = lib.hrt_render_lens_views_features.argtypes
        lib.hrt_render_denoised_guides.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                                   C.c_uint32, C.c_uint32, C.POINTER(DenoiseParams), C.c_void_p, C.POINTER(Stats)]
        lib.hrt_render_denoised_var_guides.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                                       C.c_uint32, C.c_uint32, C.POINTER(DenoiseVarParams), C.c_void_p, C.c_void_p,
                                                       C.POINTER(Stats)]
        lib.hrt_render_lit_device.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Lens), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                              C.c_uint32, C.c_uint32, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.hrt_render_lit.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Lens), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32,
                                       C.c_uint32, C.c_float, C.c_uint32, C.c_void_p, C.POINTER(Stats)]
        lib.hrt_render_lit_views_device.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(LensView), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                    C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.hrt_render_lit_views.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(LensView), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                             C.c_uint32, C.c_uint32, C.c_float, C.c_uint32, C.c_void_p, C.POINTER(Stats)]
        lib.hrt_bake_lit_device.argtypes = lib.hrt_trace_lit_paths.argtypes
        lib.hrt_bake_lit.argtypes = lib.hrt_probes_lit_paths.argtypes
        lib.hrt_render_lit_adaptive_device.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Lens), C.c_uint32, C.c_uint32, C.POINTER(Adaptive), C.c_uint64,
                                                       C.c_uint32, C.c_uint32, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.hrt_render_lit_adaptive.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Lens), C.c_uint32, C.c_uint32, C.POINTER(Adaptive), C.c_uint64,
                                                C.c_uint32, C.c_uint32, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        lib.hrt_probe_volume_blend_device.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
        lib.hrt_probe_volume_blend.argtypes = [C.c_void_p, C.c_void_p, C.c_float]
        lib.hrt_debug_pick_kernel.argtypes = [C.POINTER(PickInput), C.c_char_p, C.c_size_t]
        lib.hrt_debug_last_kernel.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        lib.hrt_debug_live_resources.argtypes = [C.POINTER(C.c_uint64 * 4)]
        lib.hrt_debug_live_resources.restype = None
        _dev = lib
    return _dev


def _fp(a):
    return np.ascontiguousarray(a, dtype=np.float32).ctypes.data_as(C.POINTER(C.c_float))


def _check(rc: int, last_error, entry: Optional[str] = None, layer: str = "hrt"):
    """The return code of a library call: ``rc``, or for a negative one HrtError with the library's last error -- "<entry> failed
    (rc): ..." for a named entry point, "<layer> error rc: ..." otherwise."""
    if rc < 0:
        raise HrtError((f"{layer} error {rc}" if entry is None else f"{entry} failed ({rc})") + f": {last_error().decode()}")
    return rc


def _call(entry: str, *args):
    """``entry`` of libhrt.so on ``args``; HrtError "<entry> failed (rc): ..." if it refuses."""
    lib = device_lib()
    return _check(getattr(lib, entry)(*args), lib.hrt_last_error, entry)


def _ref(x):
    """The argument for an optional struct: NULL for None."""
    return None if x is None else C.byref(x)


def _ptr(x):
    """The ``void*`` argument for a device buffer: a torch tensor, an address (0: NULL) or None."""
    return None if x is None else C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else x)


def _stream(device=None):
    """The ``void*`` argument for the current torch stream of ``device`` (None: of the current device)."""
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _check_tensor(who: str, name: str, t, shape, dtype: str = "float32", device=None, noun: str = "", shown: Optional[str] = None):
    """ValueError unless ``t`` is a contiguous torch tensor of ``shape`` (None: any length) and ``dtype`` ("int32" takes uint32 as
    well) on the GPU -- or, with ``device``, on that device, "the <noun>' device".  ``shown``: the shape as the message states it."""
    import torch
    dtypes = (torch.int32, torch.uint32) if dtype == "int32" else (getattr(torch, dtype),)
    if not (isinstance(t, torch.Tensor) and (t.device.type == "cuda" if device is None else t.device == device) and t.dtype in dtypes
            and t.dim() == len(shape) and all(a is None or a == b for a, b in zip(shape, t.shape)) and t.is_contiguous()):
        where = "the GPU" if device is None else f"the {noun}' device"
        raise ValueError(f"{who}: {name} must be a contiguous {shown or _shape_text(shape)} {dtype} tensor on {where}")


def _shape_text(shape) -> str:
    return "(" + ", ".join(f"{x}" for x in shape) + ")"


def _ray_batch(who: str, noun: str, batch, tensor_only: bool = False):
    """The (n, RAY_FLOATS) float32 batch of ``who`` (its rows the ``noun`` of the messages): a torch tensor on the GPU as it is,
    anything else -- unless ``tensor_only`` -- as a contiguous NumPy array; at most 2^31 - 1 rows."""
    import torch
    if tensor_only or isinstance(batch, torch.Tensor):
        _check_tensor(who, noun if tensor_only else "a torch tensor", batch, (None, RAY_FLOATS), shown="(n, 8)")
        return batch
    batch = np.ascontiguousarray(batch, dtype=np.float32)
    if batch.ndim != 2 or batch.shape[1] != RAY_FLOATS:
        raise ValueError(f"{who}: {noun} must have shape (n, {RAY_FLOATS}) (got {batch.shape})")
    return batch


def _probe_batch(who: str, noun: str, batch, tensor_only: bool = False):
    """``_ray_batch`` for probe records: (n, PROBE_FLOATS) float32."""
    import torch
    if tensor_only or isinstance(batch, torch.Tensor):
        _check_tensor(who, noun if tensor_only else "a torch tensor", batch, (None, PROBE_FLOATS), shown=f"(n, {PROBE_FLOATS})")
        return batch
    batch = np.ascontiguousarray(batch, dtype=np.float32)
    if batch.ndim != 2 or batch.shape[1] != PROBE_FLOATS:
        raise ValueError(f"{who}: {noun} must be probe records of shape (n, {PROBE_FLOATS}) (got {batch.shape})")
    return batch


def _row_count(who: str, noun: str, batch) -> int:
    n = batch.shape[0]
    if n > 0x7FFFFFFF:
        raise ValueError(f"{who}: at most 2^31 - 1 {noun} per call (got {n})")
    return n


def _batch_checked(who: str, noun: str, batch, keys, out, cell: tuple, rows=None):
    """The checks every batched entry point makes before anything is touched: ``batch`` by ``rows`` (default ``_ray_batch``),
    ``keys`` ((n,) uint32 / int32) and ``out`` ((n,) + ``cell`` float32), if given, as torch tensors on the batch's GPU or as NumPy
    -> (is the batch a torch tensor, the batch, n, the keys, the result's shape)."""
    import torch
    is_torch = isinstance(batch, torch.Tensor)
    batch = (rows or _ray_batch)(who, noun, batch)
    n = _row_count(who, noun, batch)
    shape, shown = (n,) + tuple(cell), "(n, " + ", ".join(str(c) for c in cell) + ")"
    if keys is not None:
        if is_torch:
            _check_tensor(who, "keys", keys, (n,), "int32", batch.device, noun, "(n,)")
        else:
            keys = np.ascontiguousarray(keys)
            if keys.shape != (n,) or keys.dtype not in (np.uint32, np.int32):
                raise ValueError(f"{who}: keys must be (n,) uint32 (got {keys.shape} {keys.dtype})")
    if out is not None:
        if is_torch:
            _check_tensor(who, "out", out, shape, "float32", batch.device, noun, shown)
        else:
            o = np.asarray(out)
            if o.shape != shape or o.dtype != np.float32:
                raise ValueError(f"{who}: out must be {shown} float32 (got {o.shape} {o.dtype})")
    return is_torch, batch, n, keys, shape


def _batch_on_device(is_torch: bool, batch, keys):
    """(batch, keys) as they are for torch tensors, a NumPy batch and its keys uploaded."""
    import torch
    if is_torch:
        return batch, keys
    d_batch = torch.from_numpy(batch).to("cuda")
    return d_batch, None if keys is None else torch.from_numpy(keys.view(np.int32)).to(d_batch.device)


def _batch_result(is_torch: bool, d_out, out):
    """The device result as the caller gets it: the tensor itself, or NumPy -- into ``out``, if given."""
    if is_torch:
        return d_out
    r = d_out.cpu().numpy()
    if out is not None:
        out[...] = r
        return out
    return r


def _view_table(who: str, noun: str, view_type, items, seeds):
    """(the ``view_type`` table -- View or LensView -- of ``items`` with their ``seeds`` (default 1 each), its length)."""
    items = list(items)
    n = len(items)
    seeds = [1] * n if seeds is None else [int(x) for x in seeds]
    if len(seeds) != n:
        raise ValueError(f"{who}: {n} {noun} but {len(seeds)} seeds")
    views = (view_type * max(n, 1))()
    field, item_type = view_type._fields_[0]
    for v, (item, seed) in enumerate(zip(items, seeds)):
        C.memmove(C.byref(getattr(views[v], field)), C.byref(item), C.sizeof(item_type))
        views[v].seed = seed
    return views, n


# ------------------------------------------------------------------ host scene
class HostScene:
    """Scene of the host layer (mirrors the reference's ``Scene`` set-up API)."""

    def __init__(self, asset_root: str = ASSET_ROOT):
        self._lib = host_lib()
        self._h = C.c_void_p()
        self._keep = []
        rc = self._lib.hrt_host_scene_new(asset_root.encode(), C.byref(self._h))
        self._check(rc)

    def _check(self, rc: int):
        return _check(rc, self._lib.hrt_host_last_error, layer="hrt_host")

    def close(self):
        if self._h:
            self._lib.hrt_host_scene_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def setup(self, name: str, aspect: float = 1.0, seed: int = 1) -> "HostScene":
        self._check(self._lib.hrt_host_scene_setup(self._h, name.encode(), aspect, seed))
        return self

    def clear(self):
        self._check(self._lib.hrt_host_scene_clear(self._h))
        return self

    def add_texture(self, rgb: np.ndarray) -> int:
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        return self._check(self._lib.hrt_host_scene_add_texture(self._h, rgb.shape[1], rgb.shape[0], rgb.ctypes.data))

    def add_normal_map(self, rgb: np.ndarray) -> int:
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        return self._check(self._lib.hrt_host_scene_add_normal_map(self._h, rgb.shape[1], rgb.shape[0], rgb.ctypes.data))

    def add_sphere(self, center, radius, material: Material):
        self._check(self._lib.hrt_host_scene_add_sphere(self._h, _fp(center), radius, C.byref(material)))

    def add_quad(self, bottom_left, right, up, width, height, material: Material):
        self._check(self._lib.hrt_host_scene_add_quad(self._h, _fp(bottom_left), _fp(right), _fp(up), width, height,
                                                      C.byref(material)))

    def add_mesh(self, positions: np.ndarray, indices: np.ndarray, material: Material, face_colors=None):
        p = np.ascontiguousarray(positions, dtype=np.float32)
        i = np.ascontiguousarray(indices, dtype=np.uint32)
        fc = None if face_colors is None else np.ascontiguousarray(face_colors, dtype=np.float32)
        self._check(self._lib.hrt_host_scene_add_mesh(self._h, p.ctypes.data, p.shape[0], i.ctypes.data, i.shape[0],
                                                      None if fc is None else fc.ctypes.data, C.byref(material)))

    def add_mesh_off(self, rel_path: str, material: Material):
        self._check(self._lib.hrt_host_scene_add_mesh_off(self._h, rel_path.encode(), C.byref(material)))

    def add_light(self, pos, radius, color=(1, 1, 1)):
        self._check(self._lib.hrt_host_scene_add_light(self._h, _fp(pos), radius, _fp(color)))

    def set_skybox(self, rgb: Optional[np.ndarray]):
        """Equirectangular RGB8 skybox (h, w, 3), or None to remove it (Scene::loadSkybox, from memory)."""
        if rgb is None:
            self._check(self._lib.hrt_host_scene_set_skybox(self._h, 0, 0, None))
            return
        a = np.ascontiguousarray(rgb, dtype=np.uint8)
        self._keep.append(a)
        self._check(self._lib.hrt_host_scene_set_skybox(self._h, a.shape[1], a.shape[0], a.ctypes.data))

    def set_sky(self, dark: bool):
        self._check(self._lib.hrt_host_scene_set_sky(self._h, int(dark)))

    def set_kd_params(self, leaf_max: int = 0, max_depth: int = 0):
        self._check(self._lib.hrt_host_scene_set_kd_params(self._h, leaf_max, max_depth))

    def set_kd_builder(self, fn=None, user=None):
        """hrt_host_scene_set_kd_builder: ``fn`` a hrt_kd_builder_fn (a ctypes function pointer, or an address), None = the
        host's own threaded builder.  ``set_kd_builder("gpu")`` selects libhrt.so's hrt_kd_build_gpu (needs ``init``)."""
        if fn == "gpu":
            fn = C.cast(device_lib().hrt_kd_build_gpu, C.c_void_p)
        elif fn is not None and not isinstance(fn, (int, C.c_void_p)):
            self._kd_builder_keepalive = fn  # the ctypes callback object must outlive the flatten
            fn = C.cast(fn, C.c_void_p)
        self._check(self._lib.hrt_host_scene_set_kd_builder(self._h, fn, user))
        return self

    def flatten(self) -> C.c_void_p:
        """Builds the KD-trees; returns ``const hrt_scene_desc*`` (valid until the next flatten / close)."""
        d = SceneDescPtr()
        self._check(self._lib.hrt_host_scene_flatten(self._h, C.byref(d)))
        d._owner = self
        return d

    def kd_stats(self, mesh: int = 0) -> dict:
        out = (C.c_uint32 * 6)()
        self._check(self._lib.hrt_host_scene_kd_stats(self._h, mesh, out))
        keys = ["inner", "leaves", "empty_leaves", "depth", "leaf_tri_refs", "units"]
        return dict(zip(keys, list(out)))

    def irregular_stats(self, mesh: int = 0) -> dict:
        """Triangles kept out of the SAH tree because the reference's own tree treats them specially (host/ref_tree.h)."""
        out = (C.c_uint32 * 8)()
        self._check(self._lib.hrt_host_scene_irregular_stats(self._h, mesh, out))
        return dict(zip(["out_of_tree", "slivers", "dropped", "pairs", "ref_leaves", "ref_depth", "dead", "entries"], list(out)))


def default_camera(aspect: float) -> Camera:
    cam = Camera()
    host_lib().hrt_host_default_camera(aspect, C.byref(cam))
    return cam


# ---------------------------------------------------------------- device scene
_inited = False


def init(device: int = 0):
    global _inited
    lib = device_lib()
    _check(lib.hrt_init(device), lib.hrt_last_error, f"hrt_init({device})")
    _inited = True


class DeviceScene:
    """``hrt_scene``: the flattened scene resident in HBM."""

    def __init__(self, desc: C.c_void_p):
        self._lib = device_lib()
        if not _inited:
            init(int(os.environ.get("LOCAL_RANK", "0")))
        self._h = C.c_void_p()
        self._check(self._lib.hrt_scene_create(desc, C.byref(self._h)))

    def _check(self, rc: int):
        return _check(rc, self._lib.hrt_last_error)

    def close(self):
        if self._h:
            self._lib.hrt_scene_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def render(self, cam: Camera, w: int, h: int, spp: int, seed: int = 1, flags: int = 0):
        """hrt_render: whole frame -> host ndarray (h, w, 3) float32, plus Stats."""
        out = np.empty((h, w, 3), dtype=np.float32)
        st = Stats()
        self._check(self._lib.hrt_render(self._h, C.byref(cam), w, h, spp, seed, flags, out.ctypes.data, C.byref(st)))
        return out, st

    def last_kernel(self) -> str:
        """hrt_debug_last_kernel: the name of the build this scene's last trace launch ran ("" before any)."""
        name = C.create_string_buffer(64)
        self._check(self._lib.hrt_debug_last_kernel(self._h, name, len(name)))
        return name.value.decode()

    def render_tiles(self, cam: Camera, w: int, h: int, spp: int, seed: int, flags: int, rank: int, world: int,
                     d_tiles_ptr: int, stream_ptr: int = 0):
        """hrt_render_tiles: this rank's tiles into a device buffer (asynchronous)."""
        self._check(self._lib.hrt_render_tiles(self._h, C.byref(cam), w, h, spp, seed, flags, rank, world,
                                               _ptr(d_tiles_ptr), _ptr(stream_ptr)))

    def render_accumulate(self, cam: Camera, w: int, h: int, first_sample: int, n_samples: int, seed: int, flags: int,
                          rank: int, world: int, d_sum_tiles_ptr: int, stream_ptr: int = 0):
        """hrt_render_accumulate: add samples [first_sample, first_sample + n_samples) to the running sums (asynchronous)."""
        self._check(self._lib.hrt_render_accumulate(self._h, C.byref(cam), w, h, first_sample, n_samples, seed, flags, rank,
                                                    world, _ptr(d_sum_tiles_ptr), _ptr(stream_ptr)))

    def render_adaptive(self, cam: Camera, w: int, h: int, min_spp: int, max_spp: int, threshold: float, seed: int = 1,
                        flags: int = 0, stats: Optional[Stats] = None):
        """hrt_render_adaptive: whole frame -> (frame (h, w, 3) float32, tile_spp (tiles_y, tiles_x) uint32).  Every tile of the
        frame is bit-identical to the same tile of ``render`` at that tile's count.  ``stats``: a Stats to fill, if wanted."""
        out = np.empty((h, w, 3), dtype=np.float32)
        spp = np.empty(((h + TILE - 1) // TILE, (w + TILE - 1) // TILE), dtype=np.uint32)
        p = Adaptive(min_spp, max_spp, threshold)
        self._check(self._lib.hrt_render_adaptive(self._h, C.byref(cam), w, h, C.byref(p), seed, flags, out.ctypes.data,
                                                   spp.ctypes.data, _ref(stats)))
        return out, spp

    def render_adaptive_tiles(self, cam: Camera, w: int, h: int, min_spp: int, max_spp: int, threshold: float, seed: int,
                              flags: int, rank: int, world: int, d_tiles_ptr: int, d_tile_spp_ptr: int, stream_ptr: int = 0):
        """hrt_render_adaptive_tiles: this rank's tiles (means) and their counts (uint32 per owned tile) into device buffers."""
        p = Adaptive(min_spp, max_spp, threshold)
        self._check(self._lib.hrt_render_adaptive_tiles(self._h, C.byref(cam), w, h, C.byref(p), seed, flags, rank, world,
                                                        _ptr(d_tiles_ptr), _ptr(d_tile_spp_ptr), _ptr(stream_ptr)))

    def render_features(self, cam: Camera, w: int, h: int, first_sample: int, n_samples: int, seed: int = 1) -> np.ndarray:
        """hrt_render_features: first-hit features of samples [first_sample, first_sample + n_samples) (n_samples 0: pixel centres)
        -> (h, w, FEATURE_FLOATS) float32.  The device buffer is a torch tensor on the scene's device; the call waits for it."""
        return DeviceScene._features(self, "hrt_render_features", (h, w), C.byref(cam), w, h, first_sample, n_samples, seed)

    def render_path_features(self, cam: Camera, w: int, h: int, first_sample: int, n_samples: int, seed: int = 1) -> np.ndarray:
        """hrt_render_path_features: the features of ``render_features`` taken at the FIRST DIFFUSE hit of every sample's path --
        mirror and glass followed, albedo = the throughput there, depth = the length of the chain, coverage = the fraction of
        samples that reached one (include/hrt.h "Path features") -> (h, w, FEATURE_FLOATS) float32.  ``n_samples`` >= 1."""
        return DeviceScene._features(self, "hrt_render_path_features", (h, w), C.byref(cam), w, h, first_sample, n_samples, seed)

    def _features(self, entry: str, frames: tuple, *args) -> np.ndarray:
        """What the three feature wrappers share: ``entry`` on ``args``, a fresh ``frames`` + (FEATURE_FLOATS,) device tensor and the
        current torch stream; waits, and returns the tensor as NumPy."""
        import torch
        d = torch.empty(frames + (FEATURE_FLOATS,), dtype=torch.float32, device="cuda")
        s = torch.cuda.current_stream()
        self._check(getattr(self._lib, entry)(self._h, *args, _ptr(d), C.c_void_p(s.cuda_stream)))
        s.synchronize()
        return d.cpu().numpy()

    def render_denoised(self, cam: Camera, w: int, h: int, spp: int, feature_spp: int, seed: int = 1, flags: int = 0,
                        params: Optional[DenoiseParams] = None, stats: Optional[Stats] = None, guides: str = "first") -> np.ndarray:
        """hrt_render_denoised: render, features over samples [0, feature_spp), denoise -> (h, w, 3) float32.  ``params``: a
        DenoiseParams (default values when None); ``stats``: a Stats to fill, if wanted.  ``guides``: "first", the first-hit
        features of ``render_features``, or "diffuse" (hrt_render_denoised_guides), those of ``render_path_features``, which follow
        mirror and glass to the first diffuse hit and need ``feature_spp`` >= 1."""
        g = _guides_arg("render_denoised", guides)
        out = np.empty((h, w, 3), dtype=np.float32)
        p = DenoiseParams() if params is None else params
        if g == GUIDES_FIRST_HIT:
            self._check(self._lib.hrt_render_denoised(self._h, C.byref(cam), w, h, spp, feature_spp, seed, flags, C.byref(p), out.ctypes.data,
                                                      _ref(stats)))
        else:
            self._check(self._lib.hrt_render_denoised_guides(self._h, C.byref(cam), w, h, spp, feature_spp, seed, flags, g, C.byref(p),
                                                             out.ctypes.data, _ref(stats)))
        return out

    def render_denoised_var(self, cam: Camera, w: int, h: int, spp: int, feature_spp: int, seed: int = 1, flags: int = 0,
                            params: Optional[DenoiseVarParams] = None, stats: Optional[Stats] = None, variance: bool = False,
                            guides: str = "first"):
        """hrt_render_denoised_var: render ``spp`` samples (even) keeping the first half's means, features over samples
        [0, feature_spp), the variance-guided filter -> (h, w, 3) float32; with ``variance`` the pair (frame, (h, w) float32 map of
        the result's estimated variance, in demodulated units).  ``params``: a DenoiseVarParams (default values when None).
        ``guides``: "first" or "diffuse" (hrt_render_denoised_var_guides), as ``render_denoised``."""
        g = _guides_arg("render_denoised_var", guides)
        out = np.empty((h, w, 3), dtype=np.float32)
        var = np.empty((h, w), dtype=np.float32) if variance else None
        p = DenoiseVarParams() if params is None else params
        d_var = None if var is None else var.ctypes.data
        if g == GUIDES_FIRST_HIT:
            self._check(self._lib.hrt_render_denoised_var(self._h, C.byref(cam), w, h, spp, feature_spp, seed, flags, C.byref(p),
                                                          out.ctypes.data, d_var, _ref(stats)))
        else:
            self._check(self._lib.hrt_render_denoised_var_guides(self._h, C.byref(cam), w, h, spp, feature_spp, seed, flags, g, C.byref(p),
                                                                 out.ctypes.data, d_var, _ref(stats)))
        return (out, var) if variance else out

    def render_temporal(self, history: "History", cam: Camera, w: int, h: int, spp: int, feature_spp: int, seed: int = 1, flags: int = 0,
                        tparams: Optional[TemporalParams] = None, dparams: Optional[DenoiseVarParams] = None,
                        stats: Optional[Stats] = None):
        """hrt_render_temporal: one frame of the frame loop -> (frame (h, w, 3) float32, history lengths (h, w) float32).  The frame
        of ``spp`` samples (even) is accumulated onto what ``history`` holds, reprojected from its camera, and the history is
        updated; with ``dparams`` the accumulated pair goes through the variance-guided filter, without it the accumulated frame
        is returned.  Pass a different ``seed`` every frame.  ``tparams`` None: the default TemporalParams."""
        out = np.empty((h, w, 3), dtype=np.float32)
        hist = np.empty((h, w), dtype=np.float32)
        tp = TemporalParams() if tparams is None else tparams
        self._check(self._lib.hrt_render_temporal(self._h, history._h, C.byref(cam), w, h, spp, feature_spp, seed, flags, C.byref(tp),
                                                  _ref(dparams), out.ctypes.data, hist.ctypes.data,
                                                  _ref(stats)))
        return out, hist

    def trace_rays(self, rays, mode: str = "closest", flags: int = 0, normalize: bool = False):
        """hrt_trace_rays: the scene traced with caller rays, (n, RAY_FLOATS) float32 rows {o, time, d, tmax}.

        mode "closest" -> (n, CLOSEST_FLOATS) float32 records, "shade" -> (n, SHADE_FLOATS), "occluded" -> (n,) 0 / 1 (uint32 in
        numpy, int32 in torch); the columns are HIT_* and SHADE_* above.  A contiguous float32 torch tensor on the GPU runs on the
        current torch stream of its device and gives a torch tensor there, without synchronising.  Anything else is taken as a
        NumPy array: copied to the device, traced, copied back as a NumPy array.  ``flags``: FLAG_EXACT_ONLY, FLAG_MESH_BRUTE,
        FLAG_NO_LDS_TREE; ``normalize`` adds RAYS_NORMALIZE."""
        import torch
        if mode not in _QUERY_MODES:
            raise ValueError(f"trace_rays: mode must be one of {sorted(_QUERY_MODES)} (got {mode!r})")
        q = _QUERY_MODES[mode]
        flags = int(flags) | (RAYS_NORMALIZE if normalize else 0)
        is_torch = isinstance(rays, torch.Tensor)
        rays = _ray_batch("trace_rays", "rays", rays)
        d_rays = rays if is_torch else torch.from_numpy(rays).to("cuda")
        n, dev = _row_count("trace_rays", "rays", d_rays), d_rays.device
        if q == QUERY_OCCLUDED:
            out = torch.empty((n,), dtype=torch.int32, device=dev)
        else:
            out = torch.empty((n, SHADE_FLOATS if q == QUERY_SHADE else CLOSEST_FLOATS), dtype=torch.float32, device=dev)
        self._check(self._lib.hrt_trace_rays(self._h, _ptr(d_rays), n, q, flags, _ptr(out), _stream(dev)))
        if is_torch:
            return out
        r = out.cpu().numpy()
        return r.view(np.uint32) if q == QUERY_OCCLUDED else r

    def trace_radiance(self, rays, spp: int = 1, first_sample: int = 0, seed: int = 1, keys=None, out=None, accumulate: bool = False,
                       flags: int = 0, normalize: bool = False):
        """hrt_trace_radiance: the path-traced colour of caller rays, (n, RAY_FLOATS) float32 rows {o, time, d, tmax} (tmax unused),
        samples [first_sample, first_sample + spp) of RNG stream (seed, key, sample); key i unless ``keys`` (n uint32 / int32) is given.

        Returns (n, 3) float32: the mean of the samples, or with ``accumulate`` the running sums (``out`` then holds the sums of the
        earlier samples and is updated in place).  A contiguous float32 torch tensor on the GPU runs on the current torch stream of its
        device and gives a torch tensor there, without synchronising; anything else is taken as NumPy and comes back as NumPy.
        ``flags``: FLAG_EXACT_ONLY, FLAG_MESH_BRUTE, FLAG_NO_LDS_TREE; ``normalize`` adds RAYS_NORMALIZE."""
        flags = int(flags) | (RAYS_NORMALIZE if normalize else 0) | (RADIANCE_ACCUMULATE if accumulate else 0)
        return DeviceScene._radiance_batch(self, "trace_radiance", "rays", "hrt_trace_radiance", None, rays, spp, first_sample, seed, keys,
                                           out, accumulate, flags, None)

    def _radiance_batch(self, who: str, noun: str, device_fn: str, blocking_fn: Optional[str], batch, spp, first_sample, seed, keys, out, accumulate, flags, stats,
                        rows=None, cell: tuple = (3,), extra: tuple = (), volume=None, after: tuple = ()):
        """What trace_radiance, bake and probes share: ``batch`` ((n, RAY_FLOATS) float32, the ``noun`` of the messages -- or what
        ``rows(who, noun, batch)`` accepts in place of ``_ray_batch``), ``keys`` and ``out`` ((n,) + ``cell``)
        checked as torch tensors on one GPU or as NumPy -- before ``self`` is touched -- then the entry point ``device_fn``
        (hrt_trace_radiance's signature) on the current torch stream; a NumPy batch is uploaded, and its result copied back.
        ``blocking_fn`` (hrt_bake's signature), if given, takes a NumPy batch of samples [0, spp) without ``out`` instead, and fills
        ``stats``.  ``extra``: the arguments an entry point takes between the seed and the flags (hrt_probe_depth*: r_max).
        ``volume`` (hrt_trace_lit, hrt_probes_lit*): the ProbeVolume whose handle follows the scene's; ``after``: the arguments
        between the flags and the output (eval_flags, bias)."""
        import torch
        head = (lambda: (self._h,)) if volume is None else (lambda: (self._h, volume._h))
        is_torch, batch, n, keys, shape = _batch_checked(who, noun, batch, keys, out, cell, rows)
        if out is None and accumulate and first_sample != 0:
            raise ValueError(f"{who}: accumulate after sample 0 needs the running sums in `out`")
        if blocking_fn is not None and not is_torch and out is None and not accumulate and first_sample == 0:
            r = np.empty(shape, dtype=np.float32)
            self._check(getattr(self._lib, blocking_fn)(*head(), batch.ctypes.data, None if keys is None else keys.ctypes.data, n, spp, seed, *extra, flags,
                                                        *after, r.ctypes.data, _ref(stats)))
            return r
        d_batch, d_keys = _batch_on_device(is_torch, batch, keys)
        if is_torch:
            d_out = out
        else:
            d_out = None if out is None else torch.from_numpy(np.ascontiguousarray(np.asarray(out))).to(d_batch.device)
        if d_out is None:
            d_out = torch.zeros(shape, dtype=torch.float32, device=d_batch.device)
        self._check(getattr(self._lib, device_fn)(*head(), _ptr(d_batch), _ptr(d_keys), n, first_sample, spp, seed, *extra, flags, *after, _ptr(d_out),
                                                  _stream(d_batch.device)))
        return _batch_result(is_torch, d_out, out)

    def bake(self, points, spp: int = 1, first_sample: int = 0, seed: int = 1, keys=None, out=None, accumulate: bool = False,
             flags: int = 0, stats: Optional[Stats] = None):
        """hrt_bake*: the radiance arriving at surface points, (n, RAY_FLOATS) float32 rows {P, time, N, bias}, cosine-weighted about
        N: samples [first_sample, first_sample + spp) of RNG stream (seed, key, sample); key i unless ``keys`` (n uint32 / int32).

        Returns (n, 3) float32: the mean of the samples in the units of ``trace_radiance`` (irradiance = pi x the mean radiance; no
        factor is applied), or with ``accumulate`` the running sums (``out`` then holds the sums of the earlier samples and is updated
        in place).  A contiguous float32 torch tensor on the GPU runs on the current torch stream of its device and gives a torch
        tensor there (``out``, if given, a device tensor), without synchronising (hrt_bake_device).  Anything else is taken as NumPy
        and comes back as NumPy; samples [0, spp) without ``out`` go through the blocking hrt_bake, which fills ``stats`` if given.
        ``flags``: FLAG_EXACT_ONLY, FLAG_MESH_BRUTE, FLAG_NO_LDS_TREE."""
        flags = int(flags) | (RADIANCE_ACCUMULATE if accumulate else 0)
        return DeviceScene._radiance_batch(self, "bake", "points", "hrt_bake_device", "hrt_bake", points, spp, first_sample, seed, keys, out,
                                           accumulate, flags, stats)

    def bake_lit(self, points, volume: "ProbeVolume", spp: int = 1, first_sample: int = 0, seed: int = 1, keys=None, out=None,
                 accumulate: bool = False, flags: int = 0, stats: Optional[Stats] = None, eval_flags: int = 0, bias: float = 0.0,
                 tail_after: Optional[int] = None):
        """hrt_bake_lit*: the final gather -- ``bake`` whose paths END in ``volume`` (include/hrt.h "Lit bakes") -> (n, 3) float32 in
        the units of ``bake``: sample s of a point is ``trace_lit`` of that point's record of ``bake_rays(points, s, seed, keys)``,
        in one launch for all samples and without the ray buffer.  ``tail_after`` None: one segment, the hit shaded with its own
        direct light and emission and the volume behind it; K in 1 .. MAXBOUNCES: mirror and glass followed, the volume at the K-th
        diffuse hit.  ``eval_flags`` as ``trace_lit``.  ``bias`` is the LOOK-UP's offset along the normal at the hit, as
        ``trace_lit``'s; it is not the point record's own bias float (column 7 of ``points``), which moves the ray's origin off the
        baked surface -- the two are independent.  A non-finite ``bias`` is refused here.  Everything else -- points, samples, keys,
        ``out``, ``accumulate``, ``stats``, ``flags`` and the torch (asynchronous on the current torch stream) / NumPy (blocking)
        forms -- as ``bake``.  The call only reads the volume: order an ``update`` or ``blend`` after it."""
        flags = int(flags) | (RADIANCE_ACCUMULATE if accumulate else 0)
        after = _lit_args("bake_lit", volume, eval_flags, bias) + (0 if tail_after is None else _tail_args("bake_lit", "", tail_after)[1][0],)
        return DeviceScene._radiance_batch(self, "bake_lit", "points", "hrt_bake_lit_device", "hrt_bake_lit", points, spp, first_sample, seed, keys,
                                           out, accumulate, flags, stats, volume=volume, after=after)

    def probes(self, points, spp: int = 1, first_sample: int = 0, seed: int = 1, keys=None, out=None, accumulate: bool = False,
               flags: int = 0, stats: Optional[Stats] = None):
        """hrt_probes*: the radiance arriving at points in space from every direction, (n, PROBE_FLOATS) float32 rows {P, time},
        projected onto the 9 spherical-harmonic basis functions of bands 0..2: samples [first_sample, first_sample + spp) of RNG
        stream (seed, key, sample), uniform on the sphere; key i unless ``keys`` (n uint32 / int32).

        Returns (n, PROBE_COEFFS, 3) float32: per coefficient and colour channel the mean over the samples of basis x radiance in
        the units of ``trace_radiance`` (the SH coefficients of the incoming radiance are 4 pi x 6 x the mean; no factor is applied),
        or with ``accumulate`` the running sums (``out`` then holds the sums of the earlier samples and is updated in place).  The
        sum has a fixed order (include/hrt.h "Light probes"), in blocks of PROBE_BLOCK samples.  A contiguous float32 torch tensor
        on the GPU runs on the current torch stream of its device and gives a torch tensor there (``out``, if given, a device
        tensor), without synchronising (hrt_probes_device).  Anything else is taken as NumPy and comes back as NumPy; samples
        [0, spp) without ``out`` go through the blocking hrt_probes, which fills ``stats`` if given.  Probe calls of one scene must
        not overlap each other.  ``flags``: FLAG_EXACT_ONLY, FLAG_MESH_BRUTE, FLAG_NO_LDS_TREE."""
        flags = int(flags) | (RADIANCE_ACCUMULATE if accumulate else 0)
        return DeviceScene._radiance_batch(self, "probes", "points", "hrt_probes_device", "hrt_probes", points, spp, first_sample, seed, keys, out,
                                           accumulate, flags, stats, rows=_probe_batch, cell=(PROBE_COEFFS, 3))

    def probe_depth(self, points, spp: int = 1, first_sample: int = 0, seed: int = 1, keys=None, r_max: float = 1.0, out=None,
                    accumulate: bool = False, flags: int = 0, stats: Optional[Stats] = None):
        """hrt_probe_depth*: per probe, (n, PROBE_FLOATS) float32 rows {P, time}, an 8 x 8 octahedral map of filtered depth sums
        over the directions ``probes`` uses for the same seed, keys and samples: the distance to the closest hit, at most ``r_max``
        (a miss gives ``r_max``), weighted per texel by the 32nd power of the cosine to the texel's centre direction.

        Returns (n, PROBE_DEPTH_TEXELS, 3) float32 {W, A, B}: the sums of the weights, of weight x depth and of weight x depth^2 --
        sums, not means, so that calls over further samples add up with ``accumulate`` (``out`` then holds the sums of the earlier
        samples and is updated in place).  ``ProbeVolume.update_depth`` takes them.  The sum has a fixed order (include/hrt.h
        "Probe visibility").  Torch and NumPy batches, ``out`` and ``stats`` as ``probes``.  Depth calls of one scene must not
        overlap each other.  ``flags``: FLAG_EXACT_ONLY, FLAG_MESH_BRUTE, FLAG_NO_LDS_TREE."""
        flags = int(flags) | (RADIANCE_ACCUMULATE if accumulate else 0)
        return DeviceScene._radiance_batch(self, "probe_depth", "points", "hrt_probe_depth_device", "hrt_probe_depth", points, spp, first_sample, seed,
                                           keys, out, accumulate, flags, stats, rows=_probe_batch, cell=(PROBE_DEPTH_TEXELS, 3), extra=(float(r_max),))

    def trace_lit(self, rays, volume: "ProbeVolume", spp: int = 1, first_sample: int = 0, seed: int = 1, keys=None, eval_flags: int = 0,
                  bias: float = 0.0, out=None, accumulate: bool = False, flags: int = 0, normalize: bool = False, tail_after: Optional[int] = None):
        """hrt_trace_lit: the colour of caller rays whose paths END in ``volume`` at their first hit -- the hit shaded as
        ``trace_radiance`` shades it (emission, direct light), everything beyond it the volume's irradiance about the hit's normal
        times the albedo; mirror and glass get no tail (include/hrt.h "Lit rays").  Rays, samples, keys, ``out``, ``accumulate`` and
        the torch / NumPy forms as ``trace_radiance``.  ``eval_flags``: PROBE_EVAL_FACING, LIT_VISIBLE (the look-up of
        ``ProbeVolume.eval_visible``; needs ``update_depth``); ``bias``: that look-up's offset along the normal.  Returns (n, 3)
        float32.  The call only reads the volume: order an ``update`` or ``blend`` after it.
        ``tail_after`` = K in 1 .. MAXBOUNCES (hrt_trace_lit_paths, "Lit paths"): the path is the integrator's -- mirror and glass
        followed, K - 1 diffuse bounces traced -- and ends in the volume at its K-th diffuse hit; None: the one segment above."""
        flags = int(flags) | (RAYS_NORMALIZE if normalize else 0) | (RADIANCE_ACCUMULATE if accumulate else 0)
        eval_flags, bias = _lit_args("trace_lit", volume, eval_flags, bias)
        entry, tail = _tail_args("trace_lit", "hrt_trace_lit", tail_after)
        return DeviceScene._radiance_batch(self, "trace_lit", "rays", entry, None, rays, spp, first_sample, seed, keys, out, accumulate,
                                           flags, None, volume=volume, after=(eval_flags, bias) + tail)

    def path_tails(self, rays, tail_after: int, sample: int = 0, seed: int = 1, keys=None, bias: float = 0.0, out=None, flags: int = 0,
                   normalize: bool = False):
        """hrt_path_tails: where the paths of ``trace_lit(..., tail_after=K)`` end, for ONE sample of stream (seed, key, sample) --
        (n, TAIL_FLOATS) float32 rows: [0:8] the point record {p, time, n, bias} that ``ProbeVolume.eval`` / ``eval_visible`` accept,
        [8:11] the throughput at the tail, [TAIL_WORD] a uint32 word (bits 0..7 the segments traced, TAIL_REACHED set when the path
        reached its K-th diffuse hit), [12:15] the radiance gathered so far over 6, [15] 0.  A path that ends earlier has p = n =
        thr = 0; a degenerate ray gives 16 zeros.  The value of that sample of ``trace_lit`` is [12:15] + [8:11] x the look-up of
        [0:8], bit for bit.  Rays, keys, ``flags``, ``normalize`` and the torch / NumPy forms as ``trace_radiance``; ``out``, if given,
        a tensor or array of the result's shape."""
        import torch
        who = "path_tails"
        flags, bias = int(flags) | (RAYS_NORMALIZE if normalize else 0), float(bias)
        _, tail = _tail_args(who, "hrt_path_tails", int(tail_after) if tail_after is not None else 0)
        if not np.isfinite(bias):
            raise ValueError(f"{who}: bias must be finite (got {bias})")
        is_torch, rays, n, keys, shape = _batch_checked(who, "rays", rays, keys, out, (TAIL_FLOATS,))
        d_rays, d_keys = _batch_on_device(is_torch, rays, keys)
        d_out = out if is_torch and out is not None else torch.empty(shape, dtype=torch.float32, device=d_rays.device)
        self._check(self._lib.hrt_path_tails(self._h, _ptr(d_rays), _ptr(d_keys), n, sample, seed, flags, bias, *tail, _ptr(d_out), _stream(d_rays.device)))
        return _batch_result(is_torch, d_out, out)

    def path_features(self, rays, sample: int = 0, seed: int = 1, keys=None, out=None, flags: int = 0, normalize: bool = False):
        """hrt_path_features: the path-feature record of ONE sample of stream (seed, key, sample) for every caller ray -- (n,
        FEATURE_FLOATS) float32 rows in the layout of ``render_features``: [0:3] the throughput at the path's first diffuse hit,
        [3:6] that surface's shading normal, [6:9] the emission met on the way, [9] the summed hit distances, [10] 1 where a diffuse
        hit was reached, else 0 (then [0:6] and [9] are 0 and [6:9] stays), [11] 0.  A degenerate ray gives 12 zeros.  It is
        ``path_tails(rays, 1)`` with a feature record (include/hrt.h "Path features").  Rays, keys, ``flags``, ``normalize`` and the
        torch / NumPy forms as ``trace_radiance``; ``out``, if given, a tensor or array of the result's shape."""
        import torch
        who = "path_features"
        flags = int(flags) | (RAYS_NORMALIZE if normalize else 0)
        is_torch, rays, n, keys, shape = _batch_checked(who, "rays", rays, keys, out, (FEATURE_FLOATS,))
        d_rays, d_keys = _batch_on_device(is_torch, rays, keys)
        d_out = out if is_torch and out is not None else torch.empty(shape, dtype=torch.float32, device=d_rays.device)
        self._check(self._lib.hrt_path_features(self._h, _ptr(d_rays), _ptr(d_keys), n, sample, seed, flags, _ptr(d_out), _stream(d_rays.device)))
        return _batch_result(is_torch, d_out, out)

    def probes_lit(self, points, volume: "ProbeVolume", spp: int = 1, first_sample: int = 0, seed: int = 1, keys=None, eval_flags: int = 0,
                   bias: float = 0.0, out=None, accumulate: bool = False, flags: int = 0, stats: Optional[Stats] = None,
                   tail_after: Optional[int] = None):
        """hrt_probes_lit*: ``probes`` with every sample a lit ray of ``trace_lit`` -- one segment, then ``volume`` -- in one fused
        launch: the SH9 coefficients of the light arriving at the points with one more bounce than the volume holds.  Probe records,
        samples, keys, ``out``, ``accumulate``, ``stats`` and the torch / NumPy forms as ``probes``; ``eval_flags`` and ``bias`` as
        ``trace_lit``.  Returns (n, PROBE_COEFFS, 3) float32 for ``ProbeVolume.update`` or ``.blend``.  Lit probe calls of one scene
        must not overlap each other.  ``flags``: FLAG_EXACT_ONLY, FLAG_MESH_BRUTE, FLAG_NO_LDS_TREE.  ``tail_after`` as ``trace_lit``
        (hrt_probes_lit_paths*): every sample a path that ends in the volume at its K-th diffuse hit; None: one segment."""
        flags = int(flags) | (RADIANCE_ACCUMULATE if accumulate else 0)
        eval_flags, bias = _lit_args("probes_lit", volume, eval_flags, bias)
        entry, tail = _tail_args("probes_lit", "hrt_probes_lit", tail_after)
        return DeviceScene._radiance_batch(self, "probes_lit", "points", entry + "_device", entry, points, spp, first_sample, seed,
                                           keys, out, accumulate, flags, stats, rows=_probe_batch, cell=(PROBE_COEFFS, 3), volume=volume,
                                           after=(eval_flags, bias) + tail)

    def render_views(self, cams, w: int, h: int, spp: int, seeds=None, flags: int = 0, out=None, stats: Optional[Stats] = None):
        """hrt_render_views: every camera of ``cams`` as a w x h frame of ``spp`` samples, in one launch -> (n, h, w, 3) float32;
        frame v has the bits of ``render(cams[v], w, h, spp, seeds[v], flags)``.  ``seeds``: one per view (default 1 for each, as
        ``render``).  With ``out`` a contiguous (n, h, w, 3) float32 torch tensor on the GPU the call runs on the current torch
        stream of its device without synchronising and returns ``out`` (hrt_render_views_device; ``check_last_launch`` before the
        frames are trusted).  Without it the frames come back as a NumPy array; ``stats``: a Stats to fill, if wanted."""
        views, n = _view_table("render_views", "cameras", View, cams, seeds)
        if out is not None:
            return DeviceScene._frames_device(self, "render_views", "hrt_render_views_device", (views, n, w, h, spp, flags), out, (n, h, w, 3))
        return DeviceScene._frames_blocking(self, "hrt_render_views", (views, n, w, h, spp, flags), (n, h, w, 3), stats)

    def _frames_device(self, who: str, entry: str, args: tuple, out, shape: tuple):
        """The device form ``entry`` on ``args`` into ``out``, a contiguous float32 torch tensor of ``shape`` on the GPU, on the
        current torch stream of its device, without synchronising; returns ``out``."""
        _check_tensor(who, "out", out, shape)
        self._check(getattr(self._lib, entry)(self._h, *args, _ptr(out), _stream(out.device)))
        return out

    def _frames_blocking(self, entry: str, args: tuple, shape: tuple, stats: Optional[Stats]):
        """The blocking form ``entry`` on ``args`` -> a NumPy array of ``shape``; fills ``stats`` if given."""
        frames = np.empty(shape, dtype=np.float32)
        self._check(getattr(self._lib, entry)(self._h, *args, frames.ctypes.data, _ref(stats)))
        return frames

    def _frames(self, who: str, shape: tuple, device: tuple, blocking: tuple, first_sample: int, out, accumulate: bool, stats: Optional[Stats]):
        """The frame call behind render_lens and render_lens_views; ``device`` and ``blocking``: (entry, args) of the two forms.
        ``out`` a torch tensor: the device form into it.  ``out`` NumPy, ``accumulate`` or a ``first_sample``: uploaded (or zeros),
        the device form, the result copied back (into ``out``).  Otherwise the blocking form, which fills ``stats``."""
        import torch
        if isinstance(out, torch.Tensor):
            return DeviceScene._frames_device(self, who, *device, out, shape)
        if out is not None:
            o = np.asarray(out)
            if o.shape != shape or o.dtype != np.float32:
                raise ValueError(f"{who}: out must be {_shape_text(shape)} float32 (got {o.shape} {o.dtype})")
        elif accumulate and first_sample != 0:
            raise ValueError(f"{who}: accumulate after sample 0 needs the running sums in `out`")
        if out is None and not accumulate and first_sample == 0:
            return DeviceScene._frames_blocking(self, *blocking, shape, stats)
        d = torch.zeros(shape, dtype=torch.float32, device="cuda") if out is None else torch.from_numpy(np.ascontiguousarray(o)).to("cuda")
        r = DeviceScene._frames_device(self, who, *device, d, shape).cpu().numpy()
        if out is not None:
            out[...] = r
            return out
        return r

    def render_lens(self, lens: Lens, w: int, h: int, spp: int, seed: int = 1, flags: int = 0, first_sample: int = 0, out=None,
                    accumulate: bool = False, stats: Optional[Stats] = None):
        """hrt_render_lens*: the frame of ``lens``, the mean over samples [first_sample, first_sample + spp) -> (h, w, 3) float32; with
        ``accumulate`` the running sums (``out`` then holds the sums of the earlier samples and is updated in place).  With ``out`` a
        contiguous (h, w, 3) float32 torch tensor on the GPU the call runs on the current torch stream of its device without
        synchronising and returns ``out`` (hrt_render_lens_device).  Otherwise the frame comes back as NumPy and the call blocks;
        ``stats``: a Stats to fill, if wanted (the blocking form of samples [0, spp) without ``out``: hrt_render_lens).
        ``flags``: FLAG_EXACT_ONLY, FLAG_MESH_BRUTE, FLAG_NO_LDS_TREE, FLAG_GAMMA (not with ``accumulate``)."""
        flags = int(flags) | (RADIANCE_ACCUMULATE if accumulate else 0)
        return DeviceScene._frames(self, "render_lens", (h, w, 3), ("hrt_render_lens_device", (C.byref(lens), w, h, first_sample, spp, seed, flags)),
                                   ("hrt_render_lens", (C.byref(lens), w, h, spp, seed, flags)), first_sample, out, accumulate, stats)

    def render_lens_adaptive(self, lens: Lens, w: int, h: int, min_spp: int, max_spp: int, threshold: float, seed: int = 1,
                             flags: int = 0, out=None, stats: Optional[Stats] = None):
        """hrt_render_lens_adaptive*: ``render_adaptive`` through ``lens`` -> (frame (h, w, 3) float32, tile_spp (tiles_y, tiles_x)
        uint32).  Every tile of the frame is bit-identical to the same tile of ``render_lens`` at that tile's count; with a pinhole
        lens, frame and counts are ``render_adaptive``'s.  With ``out`` a contiguous (h, w, 3) float32 torch tensor on the GPU the
        call runs on the current torch stream of its device (hrt_render_lens_adaptive_device; the stream is synchronised once per
        round) and returns ``out`` and the counts as an int32 device tensor.  Otherwise both come back as NumPy and the call blocks;
        ``stats``: a Stats to fill, if wanted (the blocking form only).  ``flags``: FLAG_EXACT_ONLY, FLAG_MESH_BRUTE, FLAG_NO_LDS_TREE,
        FLAG_GAMMA."""
        p = Adaptive(min_spp, max_spp, threshold)
        ty, tx = (h + TILE - 1) // TILE, (w + TILE - 1) // TILE
        if out is not None:
            import torch
            _check_tensor("render_lens_adaptive", "out", out, (h, w, 3))
            if stats is not None:
                raise ValueError("render_lens_adaptive: stats are the blocking form's (no `out`)")
            counts = torch.empty((ty, tx), dtype=torch.int32, device=out.device)
            self._check(self._lib.hrt_render_lens_adaptive_device(self._h, C.byref(lens), w, h, C.byref(p), seed, int(flags), _ptr(out),
                                                                  _ptr(counts), _stream(out.device)))
            return out, counts
        frame = np.empty((h, w, 3), dtype=np.float32)
        spp = np.empty((ty, tx), dtype=np.uint32)
        self._check(self._lib.hrt_render_lens_adaptive(self._h, C.byref(lens), w, h, C.byref(p), seed, int(flags), frame.ctypes.data,
                                                       spp.ctypes.data, _ref(stats)))
        return frame, spp

    def render_lens_features(self, lens: Lens, w: int, h: int, first_sample: int, n_samples: int, seed: int = 1) -> np.ndarray:
        """hrt_render_lens_features: ``render_features`` through ``lens`` -> (h, w, FEATURE_FLOATS) float32.  The device buffer is a
        torch tensor on the scene's device; the call waits for it."""
        return DeviceScene._features(self, "hrt_render_lens_features", (h, w), C.byref(lens), w, h, first_sample, n_samples, seed)

    def render_lens_path_features(self, lens: Lens, w: int, h: int, first_sample: int, n_samples: int, seed: int = 1) -> np.ndarray:
        """hrt_render_lens_path_features: ``render_path_features`` through ``lens`` -> (h, w, FEATURE_FLOATS) float32."""
        return DeviceScene._features(self, "hrt_render_lens_path_features", (h, w), C.byref(lens), w, h, first_sample, n_samples, seed)

    def render_lens_views(self, lenses, w: int, h: int, spp: int, seeds=None, flags: int = 0, first_sample: int = 0, out=None,
                          accumulate: bool = False, stats: Optional[Stats] = None):
        """hrt_render_lens_views*: every lens of ``lenses`` as a w x h frame, in one launch -> (n, h, w, 3) float32; frame v has the
        bits of ``render_lens(lenses[v], w, h, spp, seeds[v], flags, first_sample)``.  ``seeds``: one per view (default 1 for each).
        With ``accumulate`` the running sums (``out`` then holds the sums of the earlier samples and is updated in place).  With
        ``out`` a contiguous (n, h, w, 3) float32 torch tensor on the GPU the call runs on the current torch stream of its device
        without synchronising and returns ``out`` (hrt_render_lens_views_device).  Otherwise the frames come back as NumPy and the
        call blocks; ``stats``: a Stats to fill, if wanted (the blocking form of samples [0, spp) without ``out``:
        hrt_render_lens_views).  ``flags``: as ``render_lens``."""
        views, n = _view_table("render_lens_views", "lenses", LensView, lenses, seeds)
        flags = int(flags) | (RADIANCE_ACCUMULATE if accumulate else 0)
        return DeviceScene._frames(self, "render_lens_views", (n, h, w, 3), ("hrt_render_lens_views_device", (views, n, w, h, first_sample, spp, flags)),
                                   ("hrt_render_lens_views", (views, n, w, h, spp, flags)), first_sample, out, accumulate, stats)

    def render_lit(self, lens: Lens, volume: "ProbeVolume", w: int, h: int, spp: int, seed: int = 1, flags: int = 0, first_sample: int = 0,
                   out=None, accumulate: bool = False, stats: Optional[Stats] = None, eval_flags: int = 0, bias: float = 0.0,
                   tail_after: Optional[int] = None):
        """hrt_render_lit*: the frame of ``lens`` whose paths END in ``volume`` (include/hrt.h "Lit frames") -> (h, w, 3) float32:
        sample s of a pixel is ``trace_lit`` of that pixel's record of ``lens_rays(lens, w, h, s, seed)``, in one launch for all
        samples and without the ray buffer.  ``tail_after`` None: one segment, the volume at the first hit; K in 1 .. MAXBOUNCES:
        mirror and glass followed, the volume at the K-th diffuse hit.  ``eval_flags`` and ``bias`` as ``trace_lit``; everything
        else -- samples, ``out``, ``accumulate``, ``stats``, ``flags`` and the torch / NumPy forms -- as ``render_lens``.  The call
        only reads the volume: order an ``update`` or ``blend`` after it."""
        flags = int(flags) | (RADIANCE_ACCUMULATE if accumulate else 0)
        after = _lit_args("render_lit", volume, eval_flags, bias) + (0 if tail_after is None else _tail_args("render_lit", "", tail_after)[1][0],)
        return DeviceScene._frames(self, "render_lit", (h, w, 3),
                                   ("hrt_render_lit_device", (volume._h, C.byref(lens), w, h, first_sample, spp, seed, flags) + after),
                                   ("hrt_render_lit", (volume._h, C.byref(lens), w, h, spp, seed, flags) + after), first_sample, out, accumulate, stats)

    def render_lit_adaptive(self, lens: Lens, volume: "ProbeVolume", w: int, h: int, min_spp: int, max_spp: int, threshold: float, seed: int = 1,
                            flags: int = 0, out=None, stats: Optional[Stats] = None, eval_flags: int = 0, bias: float = 0.0,
                            tail_after: Optional[int] = None):
        """hrt_render_lit_adaptive*: ``render_lens_adaptive`` with the sums of ``render_lit`` (include/hrt.h "Adaptive lit frames") ->
        (frame (h, w, 3) float32, tile_spp (tiles_y, tiles_x) uint32).  Every tile of the frame is bit-identical to the same tile
        of ``render_lit`` at that tile's count.  ``eval_flags``, ``bias`` and ``tail_after`` as ``render_lit``; ``out``, ``stats``,
        ``flags`` and the torch / NumPy forms as ``render_lens_adaptive``.  The call shares the round scratch with the other
        adaptive calls of the scene (no overlap with them) and only reads the volume."""
        who = "render_lit_adaptive"
        p = Adaptive(min_spp, max_spp, threshold)
        ty, tx = (h + TILE - 1) // TILE, (w + TILE - 1) // TILE
        after = _lit_args(who, volume, eval_flags, bias) + (0 if tail_after is None else _tail_args(who, "", tail_after)[1][0],)
        if out is not None:
            import torch
            _check_tensor(who, "out", out, (h, w, 3))
            if stats is not None:
                raise ValueError(f"{who}: stats are the blocking form's (no `out`)")
            counts = torch.empty((ty, tx), dtype=torch.int32, device=out.device)
            self._check(self._lib.hrt_render_lit_adaptive_device(self._h, volume._h, C.byref(lens), w, h, C.byref(p), seed, int(flags), *after,
                                                                 _ptr(out), _ptr(counts), _stream(out.device)))
            return out, counts
        frame = np.empty((h, w, 3), dtype=np.float32)
        spp = np.empty((ty, tx), dtype=np.uint32)
        self._check(self._lib.hrt_render_lit_adaptive(self._h, volume._h, C.byref(lens), w, h, C.byref(p), seed, int(flags), *after,
                                                      frame.ctypes.data, spp.ctypes.data, _ref(stats)))
        return frame, spp

    def render_lit_views(self, lenses, volume: "ProbeVolume", w: int, h: int, spp: int, seeds=None, flags: int = 0, first_sample: int = 0,
                         out=None, accumulate: bool = False, stats: Optional[Stats] = None, eval_flags: int = 0, bias: float = 0.0,
                         tail_after: Optional[int] = None):
        """hrt_render_lit_views*: every lens of ``lenses`` as a w x h lit frame, in one launch -> (n, h, w, 3) float32; frame v has
        the bits of ``render_lit(lenses[v], volume, w, h, spp, seeds[v], ...)``.  ``seeds`` and the forms as ``render_lens_views``;
        ``eval_flags``, ``bias`` and ``tail_after`` as ``render_lit``."""
        views, n = _view_table("render_lit_views", "lenses", LensView, lenses, seeds)
        flags = int(flags) | (RADIANCE_ACCUMULATE if accumulate else 0)
        after = _lit_args("render_lit_views", volume, eval_flags, bias) + (0 if tail_after is None else _tail_args("render_lit_views", "", tail_after)[1][0],)
        return DeviceScene._frames(self, "render_lit_views", (n, h, w, 3),
                                   ("hrt_render_lit_views_device", (volume._h, views, n, w, h, first_sample, spp, flags) + after),
                                   ("hrt_render_lit_views", (volume._h, views, n, w, h, spp, flags) + after), first_sample, out, accumulate, stats)

    def render_lens_views_features(self, lenses, w: int, h: int, first_sample: int, n_samples: int, seeds=None) -> np.ndarray:
        """hrt_render_lens_views_features: ``render_lens_features`` of every lens of ``lenses`` with its seed, in one launch ->
        (n, h, w, FEATURE_FLOATS) float32.  The device buffer is a torch tensor on the scene's device; the call waits for it."""
        views, n = _view_table("render_lens_views_features", "lenses", LensView, lenses, seeds)
        return DeviceScene._features(self, "hrt_render_lens_views_features", (n, h, w), views, n, w, h, first_sample, n_samples)

    def render_lens_views_path_features(self, lenses, w: int, h: int, first_sample: int, n_samples: int, seeds=None) -> np.ndarray:
        """hrt_render_lens_views_path_features: ``render_lens_path_features`` of every lens of ``lenses`` with its seed, in one launch
        -> (n, h, w, FEATURE_FLOATS) float32."""
        views, n = _view_table("render_lens_views_path_features", "lenses", LensView, lenses, seeds)
        return DeviceScene._features(self, "hrt_render_lens_views_path_features", (n, h, w), views, n, w, h, first_sample, n_samples)

    def check_last_launch(self):
        """hrt_check_last_launch: waits for the last launch; raises if the trace kernel gave up (incomplete tiles)."""
        self._check(self._lib.hrt_check_last_launch(self._h))

    def last_kernel_ms(self) -> float:
        ms = C.c_double()
        self._check(self._lib.hrt_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value


class History:
    """``hrt_history``: what one frame of DeviceScene.render_temporal hands to the next, on the scene's device."""

    def __init__(self, scene: DeviceScene):
        self._lib = scene._lib
        self._scene = scene  # the history must not outlive its scene
        self._h = C.c_void_p()
        scene._check(self._lib.hrt_history_create(scene._h, C.byref(self._h)))

    def reset(self):
        """The next frame restarts everywhere."""
        self._lib.hrt_history_reset(self._h)

    def close(self):
        if self._h:
            self._lib.hrt_history_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _lit_args(who: str, volume, eval_flags, bias):
    """(eval_flags, bias) of a lit call, refused as include/hrt.h "Lit rays" refuses them -- before any library is touched."""
    if not isinstance(volume, ProbeVolume):
        raise ValueError(f"{who}: volume must be a ProbeVolume (got {type(volume).__name__})")
    eval_flags, bias = int(eval_flags), float(bias)
    if eval_flags & PROBE_EVAL_RADIANCE:
        raise ValueError(f"{who}: eval_flags: PROBE_EVAL_RADIANCE: the tail of a lit ray is the irradiance about the hit's normal")
    if eval_flags & ~(PROBE_EVAL_FACING | LIT_VISIBLE):
        raise ValueError(f"{who}: eval_flags: unknown bits {eval_flags & ~(PROBE_EVAL_FACING | LIT_VISIBLE)}")
    if not np.isfinite(bias):
        raise ValueError(f"{who}: bias must be finite (got {bias})")
    return eval_flags, bias


def _tail_args(who: str, entry: str, tail_after):
    """(the entry point, the arguments it takes after the bias) of a lit call: ``entry`` and nothing for ``tail_after`` None, its
    "_paths" form and K otherwise -- K refused as include/hrt.h "Lit paths" refuses it, before any library is touched."""
    if tail_after is None:
        return entry, ()
    k = int(tail_after)
    if not 1 <= k <= MAXBOUNCES:
        raise ValueError(f"{who}: tail_after must be in 1 .. {MAXBOUNCES} (got {tail_after})")
    return (entry if entry == "hrt_path_tails" else entry + "_paths"), (k,)


def _box(who: str, lo, hi):
    """``lo`` and ``hi`` of a probe grid as (3,) float32 arrays."""
    lo3, hi3 = (np.ascontiguousarray(v, dtype=np.float32) for v in (lo, hi))
    if lo3.shape != (3,) or hi3.shape != (3,):
        raise ValueError(f"{who}: lo and hi must have 3 components (got {lo3.shape} and {hi3.shape})")
    return lo3, hi3


class ProbeVolume:
    """``hrt_probe_volume``: an nx x ny x nz grid of SH9 light probes in the box ``lo`` .. ``hi`` -- the grid of ``probe_grid`` --
    that lives on the current device, to be looked up at surface points (include/hrt.h "Probe volumes").  It needs no scene."""

    def __init__(self, lo, hi, nx: int, ny: int, nz: int):
        lo3, hi3 = _box("ProbeVolume", lo, hi)
        self._h = C.c_void_p()
        self._lib = device_lib()
        self.shape = (int(nx), int(ny), int(nz))
        self.count = self.shape[0] * self.shape[1] * self.shape[2]
        self.lo, self.hi = tuple(float(x) for x in lo3), tuple(float(x) for x in hi3)
        self.loaded = False  # an update has been enqueued (relight starts a volume without one from zeros)
        _call("hrt_probe_volume_create", lo3.ctypes.data, hi3.ctypes.data, nx, ny, nz, C.byref(self._h))

    def update(self, coeffs):
        """hrt_probe_volume_update*: the coefficients of every probe, (count, PROBE_COEFFS, 3) float32 as ``DeviceScene.probes``
        returns them for ``probe_grid`` of the same box and counts.  A contiguous torch tensor on the GPU is repacked on the
        current torch stream of its device, without synchronising; anything else is taken as NumPy and uploaded."""
        import torch
        who = "ProbeVolume.update"
        is_torch = isinstance(coeffs, torch.Tensor)
        if is_torch:
            _check_tensor(who, "a torch tensor", coeffs, (None, PROBE_COEFFS, 3), shown=f"(n, {PROBE_COEFFS}, 3)")
        else:
            coeffs = np.ascontiguousarray(coeffs, dtype=np.float32)
            if coeffs.ndim != 3 or coeffs.shape[1:] != (PROBE_COEFFS, 3):
                raise ValueError(f"{who}: coeffs must have shape (n, {PROBE_COEFFS}, 3) (got {coeffs.shape})")
        if coeffs.shape[0] != self.count:
            raise ValueError(f"{who}: the volume has {self.count} probes (got coefficients of {coeffs.shape[0]})")
        if is_torch:
            with torch.cuda.device(coeffs.device):
                _call("hrt_probe_volume_update_device", self._h, _ptr(coeffs), _stream(coeffs.device))
        else:
            _call("hrt_probe_volume_update", self._h, coeffs.ctypes.data)
        self.loaded = True
        return self

    def update_depth(self, sums):
        """hrt_probe_volume_update_depth*: the depth sums of every probe, (count, PROBE_DEPTH_TEXELS, 3) float32 as
        ``DeviceScene.probe_depth`` returns them for ``probe_grid`` of the same box and counts; the volume keeps the two moments
        per texel that ``eval_visible`` reads.  Torch and NumPy as ``update``."""
        import torch
        who = "ProbeVolume.update_depth"
        is_torch = isinstance(sums, torch.Tensor)
        if is_torch:
            _check_tensor(who, "a torch tensor", sums, (None, PROBE_DEPTH_TEXELS, 3), shown=f"(n, {PROBE_DEPTH_TEXELS}, 3)")
        else:
            sums = np.ascontiguousarray(sums, dtype=np.float32)
            if sums.ndim != 3 or sums.shape[1:] != (PROBE_DEPTH_TEXELS, 3):
                raise ValueError(f"{who}: sums must have shape (n, {PROBE_DEPTH_TEXELS}, 3) (got {sums.shape})")
        if sums.shape[0] != self.count:
            raise ValueError(f"{who}: the volume has {self.count} probes (got sums of {sums.shape[0]})")
        if is_torch:
            with torch.cuda.device(sums.device):
                _call("hrt_probe_volume_update_depth_device", self._h, _ptr(sums), _stream(sums.device))
        else:
            _call("hrt_probe_volume_update_depth", self._h, sums.ctypes.data)
        return self

    def blend(self, coeffs, keep: float):
        """hrt_probe_volume_blend*: the hysteresis update of a volume that has coefficients: every coefficient becomes
        keep x old + (1 - keep) x new, ``keep`` in [0, 1).  ``coeffs`` and the torch / NumPy forms as ``update``."""
        import torch
        who = "ProbeVolume.blend"
        keep = float(keep)
        if not (0.0 <= keep < 1.0):
            raise ValueError(f"{who}: keep must be in [0, 1) (got {keep})")
        is_torch = isinstance(coeffs, torch.Tensor)
        if is_torch:
            _check_tensor(who, "a torch tensor", coeffs, (None, PROBE_COEFFS, 3), shown=f"(n, {PROBE_COEFFS}, 3)")
        else:
            coeffs = np.ascontiguousarray(coeffs, dtype=np.float32)
            if coeffs.ndim != 3 or coeffs.shape[1:] != (PROBE_COEFFS, 3):
                raise ValueError(f"{who}: coeffs must have shape (n, {PROBE_COEFFS}, 3) (got {coeffs.shape})")
        if coeffs.shape[0] != self.count:
            raise ValueError(f"{who}: the volume has {self.count} probes (got coefficients of {coeffs.shape[0]})")
        if is_torch:
            with torch.cuda.device(coeffs.device):
                _call("hrt_probe_volume_blend_device", self._h, _ptr(coeffs), keep, _stream(coeffs.device))
        else:
            _call("hrt_probe_volume_blend", self._h, coeffs.ctypes.data, keep)
        return self

    def relight(self, scene: "DeviceScene", spp: int, rounds: int, keep: float = 0.0, seed: int = 1, eval_flags: int = 0, bias: float = 0.0,
                depth_rmax: Optional[float] = None, time: float = 0.0, flags: int = 0, tail_after: Optional[int] = None):
        """The relighting loop: ``rounds`` times, ``scene.probes_lit`` at the volume's own grid points against the volume as it
        stands -- round r takes samples [r x spp, (r + 1) x spp) -- then ``update`` (``blend`` when ``keep`` > 0), all on the
        current torch stream, without synchronising.  Every round adds one bounce.  A volume that has never been updated starts from
        zero coefficients (round 0 then gathers emission and direct light alone).  With ``depth_rmax`` the depth of ``spp`` samples
        is traced and installed once before round 0 (for LIT_VISIBLE).  ``time`` is the probes' time; ``flags`` are the trace flags
        of ``probes_lit``, ``tail_after`` its argument of that name (None: one segment a sample)."""
        import torch
        who = "ProbeVolume.relight"
        spp, rounds, keep = int(spp), int(rounds), float(keep)
        if spp <= 0 or rounds < 0:
            raise ValueError(f"{who}: spp must be positive and rounds non-negative (got {spp} and {rounds})")
        if not (0.0 <= keep < 1.0):
            raise ValueError(f"{who}: keep must be in [0, 1) (got {keep})")
        if (rounds * spp) > 2 ** 32:
            raise ValueError(f"{who}: rounds x spp must be at most 2^32 (got {rounds * spp})")
        eval_flags, bias = _lit_args(who, self, eval_flags, bias)
        _tail_args(who, "hrt_probes_lit", tail_after)
        if depth_rmax is not None and not (np.isfinite(depth_rmax) and depth_rmax > 0):
            raise ValueError(f"{who}: depth_rmax must be finite and positive (got {depth_rmax})")
        points = torch.from_numpy(probe_grid(self.lo, self.hi, *self.shape, time)).to("cuda")
        if depth_rmax is not None:
            self.update_depth(scene.probe_depth(points, spp, seed=seed, r_max=float(depth_rmax), flags=flags))
        if not self.loaded:
            self.update(torch.zeros((self.count, PROBE_COEFFS, 3), dtype=torch.float32, device=points.device))
        for r in range(rounds):
            c = scene.probes_lit(points, self, spp, first_sample=r * spp, seed=seed, eval_flags=eval_flags, bias=bias, flags=flags, tail_after=tail_after)
            if keep > 0.0:
                self.blend(c, keep)
            else:
                self.update(c)
        return self

    def eval_visible(self, points, radiance: bool = False, facing: bool = False, out=None, stats: Optional[Stats] = None):
        """hrt_probe_eval_visible*: ``eval`` with every one of the eight probes also weighted by whether it can see the point --
        a Chebyshev test of the distance from the probe to P + bias x N against the two depth moments of the probe's texel in that
        direction (``update_depth``) -- so that a probe behind a wall gives at most a thousandth of its weight.  The rows' bias is
        read here; a bias that is not finite makes the point degenerate.  Arguments, result and streams as ``eval``."""
        return ProbeVolume._lookup(self, "ProbeVolume.eval_visible", "hrt_probe_eval_visible", points, radiance, facing, out, stats)

    def eval(self, points, radiance: bool = False, facing: bool = False, out=None, stats: Optional[Stats] = None):
        """hrt_probe_eval*: the volume at surface points, (n, RAY_FLOATS) float32 rows {P, time, N, bias} as ``quad_points`` and
        ``mesh_points`` write them (time and bias are not read): trilinear interpolation between the eight probes round P -- with
        ``facing``, weighted by how far each probe faces the surface -- then the irradiance / pi about N, the quantity
        ``DeviceScene.bake`` returns for the same rows, or with ``radiance`` the SH radiance arriving from direction N.

        Returns (n, 3) float32; a degenerate point gives zeros.  A contiguous float32 torch tensor on the GPU runs on the current
        torch stream of its device and gives a torch tensor there (``out``, if given, a device tensor), without synchronising
        (hrt_probe_eval_device).  Anything else is taken as NumPy and goes through the blocking hrt_probe_eval, which fills
        ``stats`` if given."""
        return ProbeVolume._lookup(self, "ProbeVolume.eval", "hrt_probe_eval", points, radiance, facing, out, stats)

    def _lookup(self, who: str, entry: str, points, radiance, facing, out, stats):
        """What eval and eval_visible share: the arguments checked before ``self`` is touched, then ``entry`` + "_device" on the
        current torch stream or the blocking ``entry``."""
        import torch
        is_torch = isinstance(points, torch.Tensor)
        points = _ray_batch(who, "points", points)
        n = _row_count(who, "points", points)
        flags = (PROBE_EVAL_RADIANCE if radiance else 0) | (PROBE_EVAL_FACING if facing else 0)
        if is_torch:
            if out is None:
                out = torch.empty((n, 3), dtype=torch.float32, device=points.device)
            else:
                _check_tensor(who, "out", out, (n, 3), "float32", points.device, "points", "(n, 3)")
            with torch.cuda.device(points.device):
                _call(entry + "_device", self._h, _ptr(points), n, flags, _ptr(out), _stream(points.device))
            return out
        if out is None:
            out = np.empty((n, 3), dtype=np.float32)
        elif not (isinstance(out, np.ndarray) and out.shape == (n, 3) and out.dtype == np.float32 and out.flags.c_contiguous):
            raise ValueError(f"{who}: out must be a contiguous (n, 3) float32 array (got {getattr(out, 'shape', None)} {getattr(out, 'dtype', None)})")
        _call(entry, self._h, points.ctypes.data, n, flags, out.ctypes.data, _ref(stats))
        return out

    def close(self):
        if self._h:
            self._lib.hrt_probe_volume_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


KAT_CAMERA, KAT_TRIANGLE, KAT_AABB, KAT_SPHERE, KAT_QUAD, KAT_OPTICS, KAT_NORMALIZE, KAT_HITWORD, KAT_DIV_KNOWN, KAT_NORMALIZE_SHARED, KAT_QUAD_RCP = range(11)
_KAT_IN = {KAT_CAMERA: 2, KAT_TRIANGLE: 7, KAT_AABB: 7, KAT_SPHERE: 7, KAT_QUAD: 7, KAT_OPTICS: 8, KAT_NORMALIZE: 3, KAT_HITWORD: 3, KAT_DIV_KNOWN: 2,
           KAT_NORMALIZE_SHARED: 3, KAT_QUAD_RCP: 7}
_KAT_OUT = {KAT_CAMERA: 12, KAT_TRIANGLE: 8, KAT_AABB: 2, KAT_SPHERE: 9, KAT_QUAD: 8, KAT_OPTICS: 8, KAT_NORMALIZE: 3, KAT_HITWORD: 4, KAT_DIV_KNOWN: 1,
            KAT_NORMALIZE_SHARED: 3, KAT_QUAD_RCP: 8}


def pick_kernel(n_meshes: int, n_lights: int, n_spheres: int, tab_rows: int, tiles: int, spp: int, flags: int = 0, has_list: bool = False,
                n_views: int = 0, kernel: str = "") -> str:
    """hrt_debug_pick_kernel: the name of the trace kernel build a launch with these traits runs (``kernel``: the value of
    HRT_KERNEL); raises HrtError where the launch would be refused.  Needs neither ``init`` nor a GPU."""
    name = C.create_string_buffer(64)
    _call("hrt_debug_pick_kernel", C.byref(PickInput(n_meshes, n_lights, n_spheres, tab_rows, tiles, spp, flags, int(has_list), n_views,
                                                     kernel.encode())), name, len(name))
    return name.value.decode()


def live_resources() -> tuple:
    """hrt_debug_live_resources: the (device buffers, pinned host buffers, events, streams) libhrt.so holds at this moment."""
    out = (C.c_uint64 * 4)()
    device_lib().hrt_debug_live_resources(C.byref(out))
    return tuple(out)


def debug_kat(which: int, inp, prim=None, cam: Optional[Camera] = None) -> np.ndarray:
    """hrt_debug_kat: the DEVICE functions of the trace path on caller vectors (include/hrt.h); returns (n, out width)."""
    a = np.ascontiguousarray(inp, dtype=np.float32).reshape(-1, _KAT_IN[which])
    out = np.empty((a.shape[0], _KAT_OUT[which]), dtype=np.float32)
    pr = None if prim is None else np.ascontiguousarray(prim, dtype=np.float32)
    _call("hrt_debug_kat", which, _ref(cam), None if pr is None else pr.ctypes.data, a.ctypes.data, a.shape[0], out.ctypes.data)
    return out


class MultiScene:
    """``hrt_multi``: one replica of the scene per slot of ``devices`` (ordinals; may repeat), image tiles across them."""

    def __init__(self, desc: C.c_void_p, devices):
        global _inited
        self._lib = device_lib()
        self._h = C.c_void_p()
        arr = (C.c_int * len(devices))(*devices)
        _check(self._lib.hrt_multi_create(desc, len(devices), arr, C.byref(self._h)), self._lib.hrt_last_error)
        self.note = self._lib.hrt_last_error().decode()  # what creation fell back from, if anything
        _inited = True

    @property
    def gather(self) -> str:
        """"rccl" (one ncclGather over the handle's communicators) or "peer" (hipMemcpyPeerAsync per slot)."""
        return self._lib.hrt_multi_gather(self._h).decode()

    def close(self):
        if self._h:
            self._lib.hrt_multi_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def render(self, cam: Camera, w: int, h: int, spp: int, seed: int = 1, flags: int = 0):
        out = np.empty((h, w, 3), dtype=np.float32)
        st = Stats()
        _check(self._lib.hrt_multi_render(self._h, C.byref(cam), w, h, spp, seed, flags, out.ctypes.data, C.byref(st)), self._lib.hrt_last_error)
        return out, st


def render_multi(desc, cam: Camera, w: int, h: int, spp: int, seed: int, flags: int, devices):
    """hrt_render_multi: create + render + destroy in one call."""
    lib = device_lib()
    out = np.empty((h, w, 3), dtype=np.float32)
    st = Stats()
    arr = (C.c_int * len(devices))(*devices)
    _check(lib.hrt_render_multi(desc, C.byref(cam), w, h, spp, seed, flags, len(devices), arr, out.ctypes.data, C.byref(st)), lib.hrt_last_error)
    return out, st


def camera_rays(cam: Camera, w: int, h: int, sample: int = 0, seed: int = 1):
    """hrt_camera_rays: the render's camera rays of sample ``sample`` of a w x h frame as a (w*h, RAY_FLOATS) float32 torch tensor
    on the current device (pixel y*w + x), written on the current torch stream.  Traced with trace_radiance(first_sample=sample)
    they give the render's samples."""
    return _frame_rays("hrt_camera_rays", cam, w, h, sample, seed)


def _frame_rays(entry: str, view, w: int, h: int, sample: int, seed: int):
    """camera_rays and lens_rays: ``entry`` on the camera or lens into a fresh (w*h, RAY_FLOATS) tensor, on the current torch stream."""
    import torch
    device_lib()  # a missing library is reported before the GPU is asked for anything
    out = torch.empty((w * h, RAY_FLOATS), dtype=torch.float32, device="cuda")
    _call(entry, C.byref(view), w, h, sample, seed, _ptr(out), _stream())
    return out


def lens_rays(lens: Lens, w: int, h: int, sample: int = 0, seed: int = 1):
    """hrt_lens_rays: the rays of sample ``sample`` of a w x h frame of ``lens`` as a (w*h, RAY_FLOATS) float32 torch tensor on the
    current device (pixel y*w + x), written on the current torch stream; a degenerate sample has direction 0.  Traced with
    trace_radiance(first_sample=sample) they give the samples of ``DeviceScene.render_lens``."""
    return _frame_rays("hrt_lens_rays", lens, w, h, sample, seed)


def bake_rays(points, sample: int = 0, seed: int = 1, keys=None):
    """hrt_bake_rays: the rays of sample ``sample`` of bake points -- a contiguous (n, RAY_FLOATS) float32 torch tensor on the GPU,
    rows {P, time, N, bias} -- as an (n, RAY_FLOATS) tensor on the same device, written on the current torch stream; a degenerate
    sample has direction 0.  ``keys``: (n,) int32 on the same device.  Traced with trace_radiance(first_sample=sample, keys=keys)
    they give the samples of ``DeviceScene.bake``."""
    import torch
    device_lib()
    _ray_batch("bake_rays", "points", points, tensor_only=True)
    n = points.shape[0]
    if keys is not None:
        _check_tensor("bake_rays", "keys", keys, (n,), "int32", points.device, "points", "(n,)")
    out = torch.empty((n, RAY_FLOATS), dtype=torch.float32, device=points.device)
    with torch.cuda.device(points.device):
        _call("hrt_bake_rays", _ptr(points), _ptr(keys), n, sample, seed, _ptr(out), _stream(points.device))
    return out


def probe_rays(points, sample: int = 0, seed: int = 1, keys=None):
    """hrt_probe_rays: the rays of sample ``sample`` of light probes -- a contiguous (n, PROBE_FLOATS) float32 torch tensor on the
    GPU, rows {P, time} -- as an (n, RAY_FLOATS) tensor on the same device, written on the current torch stream; a degenerate
    sample has direction 0.  ``keys``: (n,) int32 on the same device.  Traced with trace_radiance(first_sample=sample, keys=keys)
    they give the samples ``DeviceScene.probes`` projects."""
    import torch
    device_lib()
    _probe_batch("probe_rays", "points", points, tensor_only=True)
    n = points.shape[0]
    if keys is not None:
        _check_tensor("probe_rays", "keys", keys, (n,), "int32", points.device, "points", "(n,)")
    out = torch.empty((n, RAY_FLOATS), dtype=torch.float32, device=points.device)
    with torch.cuda.device(points.device):
        _call("hrt_probe_rays", _ptr(points), _ptr(keys), n, sample, seed, _ptr(out), _stream(points.device))
    return out


def probe_grid(lo, hi, nx: int, ny: int, nz: int, time: float = 0.0) -> np.ndarray:
    """hrt_probe_grid_points: the (nx * ny * nz, PROBE_FLOATS) float32 probe records of a regular grid in the box ``lo`` .. ``hi``,
    probe (i, j, k) at index (k * ny + j) * nx + i, at the centre of its cell.  Host only: needs no GPU."""
    lo3, hi3 = _box("probe_grid", lo, hi)
    n = int(nx) * int(ny) * int(nz)
    out = np.empty((n if 0 < n <= 0x7FFFFFFF else 1, PROBE_FLOATS), dtype=np.float32)  # a grid the library refuses writes nothing
    _call("hrt_probe_grid_points", lo3.ctypes.data, hi3.ctypes.data, nx, ny, nz, time, out.ctypes.data)
    return out


def probe_volume_weights(lo, hi, nx: int, ny: int, nz: int, point, facing: bool = False):
    """hrt_probe_volume_weights: for one point record {P, time, N, bias} (8 floats) the indices of the eight probes of an
    nx x ny x nz ``ProbeVolume`` in the box ``lo`` .. ``hi`` that ``eval`` interpolates between, and their final weights:
    ((8,) uint32, (8,) float32), both zero for a degenerate point.  Host only: needs no GPU."""
    lo3, hi3 = _box("probe_volume_weights", lo, hi)
    p = np.ascontiguousarray(point, dtype=np.float32)
    if p.shape != (RAY_FLOATS,):
        raise ValueError(f"probe_volume_weights: point must be one record of {RAY_FLOATS} floats (got {p.shape})")
    index, weight = np.zeros(8, dtype=np.uint32), np.zeros(8, dtype=np.float32)
    _call("hrt_probe_volume_weights", lo3.ctypes.data, hi3.ctypes.data, nx, ny, nz, p.ctypes.data, PROBE_EVAL_FACING if facing else 0,
          index.ctypes.data, weight.ctypes.data)
    return index, weight


def probe_depth_texel(v) -> int:
    """hrt_probe_depth_texel: the texel e = 8 j + i of a probe's octahedral depth map that the vector ``v`` (3 floats, any length
    but 0) points through, by the code the kernels run.  Needs neither ``init`` nor a GPU."""
    v3 = np.ascontiguousarray(v, dtype=np.float32)
    if v3.shape != (3,):
        raise ValueError(f"probe_depth_texel: v must have 3 components (got {v3.shape})")
    e = C.c_uint32()
    _call("hrt_probe_depth_texel", v3.ctypes.data, C.byref(e))
    return e.value


def probe_depth_direction(texel: int) -> np.ndarray:
    """hrt_probe_depth_direction: the unit centre direction of ``texel`` (below PROBE_DEPTH_TEXELS), (3,) float32."""
    out = np.empty(3, dtype=np.float32)
    _call("hrt_probe_depth_direction", int(texel), out.ctypes.data)
    return out


class _SceneDescHead(C.Structure):
    """The leading fields of ``hrt_scene_desc`` (include/hrt.h), up to the quads."""
    _fields_ = [("n_materials", C.c_uint32), ("materials", C.c_void_p), ("n_spheres", C.c_uint32), ("spheres", C.c_void_p),
                ("n_quads", C.c_uint32), ("quads", C.POINTER(Quad))]


def scene_quads(desc) -> list:
    """The quads of a flattened scene description (``HostScene.flatten()``) as copies, in the scene's order."""
    head = C.cast(desc, C.POINTER(_SceneDescHead)).contents
    return [Quad.from_buffer_copy(head.quads[i]) for i in range(head.n_quads)]


def quad_points(quad: Quad, tw: int, th: int, side: int = 1, time: float = 0.0, bias: float = 1e-4) -> np.ndarray:
    """hrt_bake_quad_points: the (tw * th, RAY_FLOATS) float32 bake points of a tw x th lightmap over ``quad``, row-major (texel
    (i, j) at j * tw + i), at the texel centres with the quad's normal times ``side`` (+1: the side the trace path lights).  Host
    only: needs no GPU."""
    n = int(tw) * int(th)
    out = np.empty((n if 0 < n <= 0x7FFFFFFF else 1, RAY_FLOATS), dtype=np.float32)  # a frame the library refuses writes nothing
    _call("hrt_bake_quad_points", C.byref(quad), tw, th, side, time, bias, out.ctypes.data)
    return out


def mesh_points(positions, indices, time: float = 0.0, bias: float = 1e-4) -> np.ndarray:
    """hrt_bake_mesh_points: one bake point per vertex of a triangle mesh -- ``positions`` (n_vertices, 3) float32, ``indices``
    (n_triangles, 3) uint32 -- with the unnormalised sum of the cross products of its triangles as the normal (0 for a vertex no
    triangle uses: a degenerate point).  Host only: needs no GPU."""
    p = np.ascontiguousarray(positions, dtype=np.float32)
    ix = np.ascontiguousarray(indices, dtype=np.uint32)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError(f"mesh_points: positions must have shape (n_vertices, 3) (got {p.shape})")
    if ix.size and (ix.ndim != 2 or ix.shape[1] != 3):
        raise ValueError(f"mesh_points: indices must have shape (n_triangles, 3) (got {ix.shape})")
    out = np.empty((p.shape[0], RAY_FLOATS), dtype=np.float32)
    _call("hrt_bake_mesh_points", p.ctypes.data, p.shape[0], ix.ctypes.data, ix.shape[0] if ix.size else 0, time, bias, out.ctypes.data)
    return out


def tiles_total(w: int, h: int) -> int:
    return ((w + TILE - 1) // TILE) * ((h + TILE - 1) // TILE)


def tiles_owned(w: int, h: int, rank: int, world: int) -> int:
    t = tiles_total(w, h)
    return (t - rank + world - 1) // world if rank < t else 0


def assemble_frame(d_gathered_ptr: int, tiles_per_rank_padded: int, w: int, h: int, world: int, d_frame_ptr: int,
                   stream_ptr: int = 0):
    _call("hrt_assemble_frame", _ptr(d_gathered_ptr), tiles_per_rank_padded, w, h, world, _ptr(d_frame_ptr), _ptr(stream_ptr))


def assemble_frame_host(gathered: np.ndarray, w: int, h: int, world: int) -> np.ndarray:
    """Host (numpy) statement of the tile -> frame mapping of hrt_assemble_frame; used by the CPU multi-rank test.

    gathered: (world, tiles_per_rank_padded, TILE*TILE, 3)."""
    tx = (w + TILE - 1) // TILE
    frame = np.zeros((h, w, 3), dtype=np.float32)
    for t in range(tiles_total(w, h)):
        rank, slot = t % world, t // world
        x0, y0 = (t % tx) * TILE, (t // tx) * TILE
        tile = gathered[rank, slot].reshape(TILE, TILE, 3)
        hh, ww = min(TILE, h - y0), min(TILE, w - x0)
        frame[y0:y0 + hh, x0:x0 + ww] = tile[:hh, :ww]
    return frame


def finalize_tiles(d_sum_tiles_ptr: int, n_tiles: int, total_samples: int, flags: int, d_tiles_ptr: int, stream_ptr: int = 0):
    """hrt_finalize_tiles: running sums -> pixel means (+ gamma with FLAG_GAMMA); the two pointers may be equal."""
    _call("hrt_finalize_tiles", _ptr(d_sum_tiles_ptr), n_tiles, total_samples, flags, _ptr(d_tiles_ptr), _ptr(stream_ptr))


def denoise_scratch_bytes(w: int, h: int) -> int:
    """hrt_denoise_scratch_bytes: size of the scratch buffer hrt_denoise needs for a w x h frame."""
    return int(device_lib().hrt_denoise_scratch_bytes(w, h))


def denoise(d_color_ptr: int, d_features_ptr: int, w: int, h: int, params: Optional[DenoiseParams], flags: int, d_scratch_ptr: int,
            d_out_ptr: int, stream_ptr: int = 0):
    """hrt_denoise on device pointers (asynchronous on the stream): linear colour (h, w, 3) and features (h, w, FEATURE_FLOATS)
    -> d_out (h, w, 3).  ``params`` None: the default DenoiseParams; ``flags``: FLAG_GAMMA or 0."""
    p = DenoiseParams() if params is None else params
    _call("hrt_denoise", _ptr(d_color_ptr), _ptr(d_features_ptr), w, h, C.byref(p), flags, _ptr(d_scratch_ptr), _ptr(d_out_ptr), _ptr(stream_ptr))


def denoise_var_scratch_bytes(w: int, h: int) -> int:
    """hrt_denoise_var_scratch_bytes: size of the scratch buffer hrt_denoise_var needs for a w x h frame."""
    return int(device_lib().hrt_denoise_var_scratch_bytes(w, h))


def denoise_var(d_color_ptr: int, d_color_half_ptr: int, d_features_ptr: int, w: int, h: int, params: Optional[DenoiseVarParams],
                flags: int, d_scratch_ptr: int, d_out_ptr: int, d_variance_out_ptr: int = 0, stream_ptr: int = 0):
    """hrt_denoise_var on device pointers (asynchronous on the stream): linear means of all samples and of their first half
    (h, w, 3) and features (h, w, FEATURE_FLOATS) -> d_out (h, w, 3) and, if its pointer is not 0, the variance map (h, w).
    ``params`` None: the default DenoiseVarParams; ``flags``: FLAG_GAMMA or 0."""
    p = DenoiseVarParams() if params is None else params
    _call("hrt_denoise_var", _ptr(d_color_ptr), _ptr(d_color_half_ptr), _ptr(d_features_ptr), w, h, C.byref(p), flags, _ptr(d_scratch_ptr),
          _ptr(d_out_ptr), _ptr(d_variance_out_ptr), _ptr(stream_ptr))


def temporal_accumulate(cam: Camera, prev_cam: Optional[Camera], w: int, h: int, d_color_ptr: int, d_color_half_ptr: int, d_features_ptr: int,
                        d_prev_color_ptr: int, d_prev_color_half_ptr: int, d_prev_features_ptr: int, d_prev_history_ptr: int,
                        params: Optional[TemporalParams], d_out_ptr: int, d_out_half_ptr: int, d_history_out_ptr: int, stream_ptr: int = 0):
    """hrt_temporal_accumulate on device pointers (asynchronous on the stream): the current frame's linear means, first-half means
    (0: none) and features, the previous call's outputs with the features and camera of that frame (``prev_cam`` None and 0s: the
    first frame) -> accumulated colour, half colour and history lengths.  ``params`` None: the default TemporalParams."""
    p = TemporalParams() if params is None else params
    _call("hrt_temporal_accumulate", C.byref(cam), _ref(prev_cam), w, h, _ptr(d_color_ptr), _ptr(d_color_half_ptr), _ptr(d_features_ptr),
          _ptr(d_prev_color_ptr), _ptr(d_prev_color_half_ptr), _ptr(d_prev_features_ptr), _ptr(d_prev_history_ptr), C.byref(p), _ptr(d_out_ptr),
          _ptr(d_out_half_ptr), _ptr(d_history_out_ptr), _ptr(stream_ptr))


def encode_ppm(d_frame_ptr: int, w: int, h: int, fmt: int, d_out_ptr: int, capacity: int, stream_ptr: int = 0) -> int:
    """hrt_encode_ppm: the reference's PPM file (fmt 3, byte for byte) or its binary form (fmt 6), encoded on the
    device into d_out; returns the file size in bytes."""
    n = C.c_size_t(0)
    _call("hrt_encode_ppm", _ptr(d_frame_ptr), w, h, fmt, _ptr(d_out_ptr), capacity, C.byref(n), _ptr(stream_ptr))
    return int(n.value)


def ppm_text_reference(rgb: np.ndarray) -> bytes:
    """Host statement of main.cpp:258-262 (what `ofstream <<` writes for an (h, w, 3) float32 frame); the
    checker of hrt_encode_ppm in the tests."""
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    h, w, _ = rgb.shape
    m = np.where(rgb < np.float32(1.0), rgb, np.float32(1.0))          # std::min<float>(1.f, c): NaN -> 1
    v = (np.float32(255.0) * m).astype(np.float32)
    with np.errstate(invalid="ignore"):
        iv = np.where(np.isfinite(v), np.trunc(np.clip(v, -2147483648.0, 255.0)), -2147483648.0).astype(np.int64)
    body = " ".join(str(int(x)) for x in iv.reshape(-1))
    return f"P3\n{w} {h}\n255\n".encode() + body.encode() + b" \n"


def write_ppm(path: str, rgb: np.ndarray):
    """P3 dump with the reference's quantisation (main.cpp:258-261)."""
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    _call("hrt_write_ppm", path.encode(), rgb.ctypes.data, rgb.shape[1], rgb.shape[0])
