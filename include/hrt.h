/*
 * hrt.h -- C ABI of the MI355X ray-trace path (libhrt.so).
 *
 * This is the drop-in boundary for the reference's 'r'-triggered render:
 *   key 'r'                         /root/reference/main.cpp:321-325
 *   void ray_trace_from_camera()    /root/reference/main.cpp:200-263
 *     -> trace_line()               /root/reference/main.cpp:183-198
 *        -> Scene::rayTrace()       /root/reference/src/Scene.h:345-350
 * The reference has no FFI of its own; a maintainer replaces
 * the body of ray_trace_from_camera() with: flatten scene -> hrt_scene_create
 * -> hrt_render -> PPM dump.
 *
 * Everything here is plain C: pointers, sizes, PODs.  No torch / HIP types.
 * All functions return 0 on success or a negative hrt_status; they never
 * throw.  hrt_last_error() gives the text of the last failure on the calling
 * thread.  Calls are blocking unless a stream is given.
 */
#ifndef HRT_H
#define HRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* libhrt.so is built with -fvisibility=hidden: the functions declared here are everything it exports. */
#define HRT_API __attribute__((visibility("default")))

/* ---- compile-time constants of the path (reference src/Constants.h) ---- */
#define HRT_MAXBOUNCES 6             /* Constants.h:11  MAXBOUNCES            */
#define HRT_NB_ECH 10                /* Constants.h:12  shadow rays per light  */
#define HRT_EPSILON 0.00001          /* Constants.h:18  (a double literal)     */
#define HRT_TRIANGLE_SCALING 1.000001f /* Mesh.h:23                             */

typedef enum hrt_status {
    HRT_OK = 0,
    HRT_ERR_INVALID = -1,   /* bad argument / inconsistent scene description   */
    HRT_ERR_DEVICE = -2,    /* HIP runtime failure (no GPU, OOM, launch error) */
    HRT_ERR_STATE = -3,     /* library not initialised / scene destroyed       */
    HRT_ERR_IO = -4         /* file could not be read / written                */
} hrt_status;

/* Material.h:11-21 */
enum { HRT_MAT_DIFFUSE = 0, HRT_MAT_GLASS = 1, HRT_MAT_MIRROR = 2 };
enum { HRT_TEX_NONE = 0, HRT_TEX_CHECKER = 1, HRT_TEX_IMAGE = 2 };
/* Mesh.h:64-68 */
enum { HRT_COLOR_VERTEX = 0, HRT_COLOR_FACE = 1, HRT_COLOR_NONE = 2 };

/* The fields of reference `struct Material` (Material.h:23-50) that the hot
 * path reads.  ambient/specular/shininess are never read by the integrator
 * (Scene.h:317 is commented out) and are not carried. */
typedef struct hrt_material {
    float albedo[3];          /* diffuse_material                              */
    float transparency;
    float index_medium;
    int32_t type;             /* HRT_MAT_*                                      */
    int32_t texture_type;     /* HRT_TEX_*                                      */
    float checker1[3];
    float checker2[3];
    float tex_scale_x, tex_scale_y;
    int32_t emissive;         /* 0/1; undefined in the reference => 0 (N10)     */
    float light_color[3];
    float light_intensity;
    int32_t image;            /* index into images[], -1 = none                 */
    int32_t normal_map;       /* index into images[], -1 = no normal map        */
    float motion[3];          /* motion_blur_translation                        */
} hrt_material;

/* ppmLoader::ImageRGB (imageLoader.h:18-22): tightly packed RGB8, row-major. */
typedef struct hrt_image {
    int32_t w, h;
    const uint8_t *rgb;
} hrt_image;

/* Sphere.h:45-47 */
typedef struct hrt_sphere {
    float center[3];
    float radius;
    int32_t material;
} hrt_sphere;

/* Square: intersect() reads vertices[0],[1],[3] (Square.h:68-70); the normal
 * map frame is m_right_vector / m_up_vector as left by setQuad (Square.h:35-45,
 * Scene.h:284), which later transforms do NOT update. */
typedef struct hrt_quad {
    float v0[3], v1[3], v3[3];
    float tangent[3], bitangent[3];
    int32_t material;
} hrt_quad;

/* Scene.h:28-41; only pos/radius/material are read (Scene.h:306-333). */
typedef struct hrt_light {
    float pos[3];
    float radius;
    float color[3];
} hrt_light;

/* Flattened KD-tree with ropes, in 16-byte units ("nodelets").
 *   ref = unit index | HRT_KD_LEAF (leaf) ; HRT_KD_NIL = no neighbour.
 *   inner nodelet (1 unit):  { f32 split, u32 axis, u32 left_ref, u32 right_ref }
 *   leaf  nodelet (4 units): { bmin.xyz, u32 tri_first | bmax.xyz, u32 tri_count |
 *                              rope[-x,+x,-y,+y] | rope[-z,+z], 0, 0 }
 * tri_first/tri_count index leaf_tris[] (triangle ids of the mesh).
 * Any numbering is valid: hrt_scene_create re-lays the reachable part of the tree for its walk (two-level treelets,
 * breadth-first, so that a prefix of ITS array is the top of the tree -- what the kernels stage into LDS).  The host
 * builder keeps a node and its inner children inside one 64-byte line and starts leaves on 64-byte boundaries (unused
 * padding units are zero), which is what the CPU-side walks of the same array like. */
#define HRT_KD_LEAF 0x80000000u
#define HRT_KD_NIL 0xFFFFFFFFu
typedef struct hrt_kdunit {
    uint32_t w[4];
} hrt_kdunit;

/* The SPLIT SEARCH of the tree build as a replaceable step ("GPU (or parallel host) flattened KD build with
 * SAH", replacing KDTree::buildTree, KDTree.cpp:87-151).  The host layer prepares the triangle references of a mesh
 * (id + bounds, the padded root cell, the heuristic's constants), hands them to a builder, and turns the builder's nodes
 * into the rope tree of hrt_kdunit above.  Two builders exist and give the SAME nodes: the host's own (threaded, the
 * default) and hrt_kd_build_gpu in libhrt.so (level by level on the device); hrt_host_scene_set_kd_builder selects.
 * The host layer hands a builder no -0.0 in lo / hi (it becomes +0.0), and a builder treats a -0.0 it is given as +0.0: the
 * two compare equal, so otherwise the sign of a split at zero would depend on the order of the references.  tests/kd_ref.py
 * states the whole rule in numpy. */
typedef struct hrt_kd_build_input {
    uint32_t n_refs;
    const uint32_t *ids;   /* triangle id of each reference                                                  */
    const float *lo, *hi;  /* 3 floats per reference: bounds of the triangle (of the part inside the cell)   */
    float cell_lo[3], cell_hi[3];  /* the root cell (padded hull)                                            */
    uint32_t leaf_max, max_depth;  /* a node of <= leaf_max references, or at depth max_depth, is a leaf     */
    float cost_traverse, cost_intersect, empty_bonus;  /* surface-area heuristic                              */
} hrt_kd_build_input;
typedef struct hrt_kd_build_node {
    int32_t axis;          /* 0..2: inner node, -1: leaf                                                     */
    float split;
    int32_t left, right;   /* inner: indices into nodes[]                                                    */
    float lo[3], hi[3];    /* the node's cell                                                                */
    uint32_t first_tri, n_tris;  /* leaf: its triangle ids are tris[first_tri .. first_tri + n_tris), ascending */
} hrt_kd_build_node;
typedef struct hrt_kd_build_output {   /* arrays allocated by the builder with malloc(); the caller free()s them */
    hrt_kd_build_node *nodes;
    uint32_t n_nodes;
    uint32_t *tris;
    uint32_t n_tris;
    int32_t root;
    uint32_t depth;        /* deepest node */
} hrt_kd_build_output;
typedef int (*hrt_kd_builder_fn)(const hrt_kd_build_input *in, hrt_kd_build_output *out, void *user);

/* IRREGULAR triangles (hai719-raytracing_amd/host/ref_tree.h).  The reference only finds a triangle through the leaves of
 * its own KD-tree (KDTree.cpp:31-69): a ray tests it when it passes the box of a leaf that holds it.  That is
 * unobservable except for triangles its builder drops below depth 100 (KDTree.cpp:101) and for
 * near-degenerate slivers, whose barycentric test (Triangle.h:62-75) accepts phantom points far outside the triangle.
 * Those triangles are kept OUT of the flattened tree (not listed in leaf_tris) and tested exactly when the reference
 * would: when AABB::intersects (AABB.h:48-65) passes for the box of one of the reference leaves that hold them.
 * One entry per (triangle, reference leaf, box) -- a leaf is one box, or a few when ancestors stick in (`group`) -- in any
 * order; hrt_scene_create groups them by triangle under a small bounding hierarchy: a ray tests such a triangle at most once,
 * and asks its boxes only for a hit closer than the best. */
typedef struct hrt_tri_exception {
    uint32_t triangle;           /* triangle id of the mesh */
    float box_min[3], box_max[3];
    uint32_t group;              /* which reference leaf this box belongs to: the entries of one triangle with the same group are the
                                    boxes the ray must ALL pass to reach that leaf -- the leaf's own box, and those of its ancestors
                                    that do not contain it (the reference cuts a node at the median of UNCLIPPED triangle bounds,
                                    KDTree.cpp:87-98: the plane can lie outside the node and a child then sticks out of its parent).
                                    The triangle is tested when some group passes entirely.                                        */
} hrt_tri_exception;

typedef struct hrt_mesh {
    uint32_t n_vertices, n_triangles;
    const float *positions;      /* 3*n_vertices, world space, NOT yet scaled by
                                    HRT_TRIANGLE_SCALING (KDTree.cpp:38-40)      */
    const uint32_t *indices;     /* 3*n_triangles                               */
    int32_t color_type;          /* HRT_COLOR_*                                 */
    const float *vert_colors;    /* 3*n_vertices or NULL                        */
    const float *face_colors;    /* 3*n_triangles or NULL                       */
    float aabb_min[3], aabb_max[3]; /* Mesh::computeAABB (Mesh.h:143-157)       */
    int32_t material;
    /* flattened KD-tree (built by the host layer, hrt_host.h) */
    uint32_t kd_root;            /* ref of the root                             */
    float kd_min[3], kd_max[3];  /* root cell of the tree (scaled-triangle hull, padded) */
    uint32_t n_kd_units;
    const hrt_kdunit *kd_units;
    uint32_t n_leaf_tris;
    const uint32_t *leaf_tris;
    /* irregular triangles (may be 0 / NULL: then every triangle must be in the tree) */
    uint32_t n_exceptions;
    const hrt_tri_exception *exceptions;
} hrt_mesh;

/* Limits hrt_scene_create enforces (HRT_ERR_INVALID, hrt_last_error() names the one that was passed): at most 32 meshes (the
 * mask of the meshes a ray has still to walk is 32 bits), and at most HRT_MAX_SOUP_SLOTS rows in the triangle soup of all meshes
 * together -- n_leaf_tris of every mesh plus one row per irregular triangle, which is counted by its bound min(n_exceptions,
 * n_triangles) so that the limit is checked before any array is read.  A path record of the streaming kernel names the triangle of
 * its closest hit by soup slot in 25 bits, beside the hit's kind and mesh in one word. */
#define HRT_MAX_SOUP_SLOTS (1u << 25)
typedef struct hrt_scene_desc {
    uint32_t n_materials;  const hrt_material *materials;
    uint32_t n_spheres;    const hrt_sphere *spheres;
    uint32_t n_quads;      const hrt_quad *quads;
    uint32_t n_meshes;     const hrt_mesh *meshes;
    uint32_t n_lights;     const hrt_light *lights;
    uint32_t n_images;     const hrt_image *images;
    int32_t dark_sky;      /* Scene.h:65                                        */
    int32_t skybox_image;  /* index into images[] or -1 (Scene.h:149-161)       */
} hrt_scene_desc;

/* Replaces the GL read-back of matrixUtilities.h:33-74: eye + orthonormal
 * basis + the gluPerspective parameters of Camera.cpp:24-28,41-50.
 * Reference default: eye (0,0,6.1), right +X, up +Y, forward -Z, fovy 45,
 * znear 4.1, zfar 1e4, aspect = w/h. */
typedef struct hrt_camera {
    float eye[3];
    float right[3], up[3], forward[3];
    float fovy_deg;
    float aspect;
    float znear, zfar;
} hrt_camera;

/* Image-tile partition of one frame across ranks (one process per GPU).
 * Tiles are HRT_TILE x HRT_TILE pixels, numbered row-major; rank r renders
 * tiles r, r+world, r+2*world, ... and writes them densely, tile-major, into
 * its own buffer (hrt_tiles_owned() tiles of HRT_TILE*HRT_TILE*3 floats). */
#define HRT_TILE 8

enum {
    HRT_FLAG_GAMMA = 1u,       /* apply pow(c,1/2.2) (main.cpp:196)             */
    HRT_FLAG_NO_LDS_TREE = 2u, /* debug: fetch every nodelet from global memory */
    HRT_FLAG_WAVE_KERNEL = 4u, /* force the one-pixel-per-lane kernel                                             */
    HRT_FLAG_STREAM_KERNEL = 8u, /* force the workgroup-streaming kernel (the default for scenes with meshes or lights) */
    HRT_FLAG_NO_SHADOW_CULL = 16u, /* debug: shadow rays test every sphere (the reference's loop) instead of the culled groups */
    HRT_FLAG_DUAL_KERNEL = 32u, /* force the two-streams-per-lane kernel (mesh scenes; all kernel forms give identical pixels) */
    /* Proof builds of the lane-per-pixel and streaming kernels: no filter and no reciprocal approximation anywhere in
     * front of the reference arithmetic.  Every square goes through Square::intersect's arithmetic in index order
     * (Square.h:65-126, Scene.h:214-221), every mesh gate through AABB::intersects' fp64 form (AABB.h:48-65,
     * KDTree.cpp:82), shadow rays test every sphere (Scene.h:235-255), the camera quotient is a true fp64 division
     * (matrixUtilities.h:66-68).  Slow; exists so tests can show that the default path's filters never change a pixel. */
    HRT_FLAG_EXACT_ONLY = 64u,
    /* With HRT_FLAG_EXACT_ONLY: meshes are not walked through the KD-tree at all -- every triangle of a gated mesh is
     * tested (Mesh::intersectOld, Mesh.h:257-277).  Shows that the rope walk never skips the closest triangle. */
    HRT_FLAG_MESH_BRUTE = 128u
};

typedef struct hrt_stats {
    double kernel_ms;          /* HIP-event time of the trace kernel(s)         */
    double total_ms;           /* wall time of the call                         */
    uint64_t samples;          /* pixels * spp rendered by this call            */
    uint32_t vgprs, sgprs, lds_bytes, waves_launched;
} hrt_stats;

typedef struct hrt_scene hrt_scene;   /* opaque: device-resident SoA scene */

/* Prepares `device_ordinal` (once) and makes it the current device of the library: scenes are created on the current
 * device and stay there.  May be called for several devices.  Entry points that take an hrt_scene or an hrt_multi switch
 * the calling thread to that scene's device (every time: HIP's current device is per thread) and leave it current.
 * Entry points that only take device POINTERS -- hrt_assemble_frame, hrt_finalize_tiles, hrt_encode_ppm -- and the
 * scene-less debug calls (hrt_debug_kat, hrt_debug_path_stream) do not switch: they run on the calling thread's current
 * device, which must be the one the pointers live on. */
HRT_API int hrt_init(int device_ordinal);
HRT_API void hrt_shutdown(void);
HRT_API const char *hrt_last_error(void);
HRT_API int hrt_device_count(void);

/* Upload: repack the description into device SoA arrays (checked and packed on the host by
 * csrc/hrt_pack.h pack_scene, which needs no device; then uploaded).  The description
 * (and everything it points to) may be freed after the call returns. */
HRT_API int hrt_scene_create(const hrt_scene_desc *desc, hrt_scene **out);
HRT_API void hrt_scene_destroy(hrt_scene *scene);

/* Whole frame on the current device into a HOST buffer out_rgb[h*w*3]
 * (row-major x + y*w, as main.cpp:193).  Value = mean over spp of
 * Scene::rayTrace, gamma-corrected when HRT_FLAG_GAMMA. */
HRT_API int hrt_render(hrt_scene *scene, const hrt_camera *cam, uint32_t w, uint32_t h,
               uint32_t spp, uint64_t seed, uint32_t flags, float *out_rgb,
               hrt_stats *stats /* may be NULL */);

/* Several GPUs from ONE process -- the multi-GPU form of the reference's single caller ray_trace_from_camera()
 * (main.cpp:200-263).  Slot i of `device_ordinals` holds a replica of the scene on that device, renders the image tiles
 * i, i + n, i + 2n, ... on a stream of its own (all slots run at once), and its dense tile buffer travels device to
 * device (xGMI between GPUs) into its block of a gather buffer on slot 0's device: ONE gather step -- an RCCL gather, or
 * peer copies, see hrt_multi_gather -- and no reduction (slots own disjoint pixels).  Slot 0 then de-interleaves the tiles and copies the frame to out_rgb (host, h*w*3).  The pixels
 * are bit-identical to hrt_render's for any number of slots.  An ordinal may be repeated (several slots share a GPU),
 * which makes the path testable on a one-GPU machine.  hrt_multi_create prepares every listed device (hrt_init is not
 * needed first) and leaves slot 0's device current; stats: kernel_ms = the slowest slot's kernel.
 * hrt_render_multi = create + render + destroy in one call. */
typedef struct hrt_multi hrt_multi;
HRT_API int hrt_multi_create(const hrt_scene_desc *desc, uint32_t n_devices, const int *device_ordinals, hrt_multi **out);
HRT_API int hrt_multi_render(hrt_multi *m, const hrt_camera *cam, uint32_t w, uint32_t h, uint32_t spp, uint64_t seed,
                     uint32_t flags, float *out_rgb, hrt_stats *stats /* may be NULL */);
HRT_API void hrt_multi_destroy(hrt_multi *m);
/* Which gather this handle runs: "rccl" -- one ncclGather (rccl.h:745) to slot 0 over the communicators hrt_multi_create
 * made with ncclCommInitAll, the default whenever the ordinals are distinct (one slot included) -- or "peer" --
 * hipMemcpyPeerAsync per slot, used when an ordinal repeats or when HRT_MULTI_GATHER=peer is set in the environment
 * (HRT_MULTI_GATHER=rccl makes a missing librccl.so or a failed communicator an error instead of a fallback).  After a
 * successful hrt_multi_create, hrt_last_error() holds a note about anything that was fallen back from (else ""). */
HRT_API const char *hrt_multi_gather(const hrt_multi *m);
HRT_API int hrt_render_multi(const hrt_scene_desc *desc, const hrt_camera *cam, uint32_t w, uint32_t h, uint32_t spp,
                     uint64_t seed, uint32_t flags, uint32_t n_devices, const int *device_ordinals, float *out_rgb,
                     hrt_stats *stats /* may be NULL */);

/* Multi-GPU building blocks (device pointers; `stream` is a hipStream_t cast
 * to void*, NULL = the default stream).  Asynchronous w.r.t. the host. */
HRT_API uint32_t hrt_tiles_total(uint32_t w, uint32_t h);
HRT_API uint32_t hrt_tiles_owned(uint32_t w, uint32_t h, uint32_t rank, uint32_t world);
HRT_API int hrt_render_tiles(hrt_scene *scene, const hrt_camera *cam, uint32_t w,
                     uint32_t h, uint32_t spp, uint64_t seed, uint32_t flags,
                     uint32_t rank, uint32_t world,
                     float *d_tiles /* device, hrt_tiles_owned()*HRT_TILE^2*3 */,
                     void *stream);
/* Rank 0 after the gather: d_gathered holds world blocks of
 * tiles_per_rank_padded tiles (rank-major); writes the row-major frame. */
HRT_API int hrt_assemble_frame(const float *d_gathered, uint32_t tiles_per_rank_padded,
                       uint32_t w, uint32_t h, uint32_t world,
                       float *d_frame /* device, h*w*3 */, void *stream);
/* One hrt_scene carries one launch at a time (it owns the work-queue head, the path pool and the camera block of the
 * launch).  Launches of the same scene on ONE stream are ordered by the stream; a launch on a different stream is made
 * to wait for the previous one.  Two scenes never interfere.  A batched launch (hrt_render_views*, below) uses the same work-queue
 * head and path pool, with its per-view blocks in place of the camera block: it is ordered against the other launches of its
 * scene exactly as an hrt_render_tiles on its stream is, and hrt_check_last_launch / hrt_last_kernel_ms speak of it when it was
 * the last.
 *
 * hrt_check_last_launch: waits for the last launch of this scene and returns HRT_ERR_DEVICE when the trace kernel gave
 * up (its scheduler has a cycle bound so that a bug can never spin the GPU): the tiles of that launch are then
 * incomplete and must not be used.  hrt_render and hrt_last_kernel_ms call it themselves; callers of the asynchronous
 * entry points (hrt_render_tiles, hrt_render_accumulate) call it before they consume or ship the tiles. */
HRT_API int hrt_check_last_launch(hrt_scene *scene);
/* Timing of the last hrt_render_tiles on this scene (after a sync). */
HRT_API int hrt_last_kernel_ms(hrt_scene *scene, double *ms);
HRT_API int hrt_kernel_info(hrt_stats *out);

/* Parity instruments (deterministic, no RNG): first-hit AOVs through pixel
 * centres at time 0.  which: 0 = (t, kind, index) with kind 1 sphere / 2 square /
 * 3 mesh and index = object or triangle id (t = 0, index = -1 on a miss),
 * 1 = shading normal, 2 = albedo, 3 = emission.  out_rgb: host, h*w*3. */
HRT_API int hrt_render_aov(hrt_scene *scene, const hrt_camera *cam, uint32_t w, uint32_t h,
                   uint32_t which, float *out_rgb);
/* Draws 0..n-1 of the per-path RNG stream (seed, pixel, sample) as the kernel
 * produces them (DESIGN.md "RNG stream").  out: host, n floats. */
HRT_API int hrt_debug_path_stream(uint64_t seed, uint32_t pixel, uint32_t sample, uint32_t n, float *out);

/* Known-answer instrument: runs the DEVICE functions of the trace path on caller vectors (one lane each), so that a test
 * can compare the device arithmetic bit for bit with vectors produced by the reference's own code instead of inferring
 * it from pixels.  `in` holds n rows, `out` receives n rows (host memory); rays are {origin, direction, time} and get
 * the Ray constructor's normalisation (Line.h:13-16).
 *   which             cam / prim                                in row   out row
 *   HRT_KAT_CAMERA    cam                                       u, v     12: Ray origin + direction (main.cpp:189-192,
 *                                                                        matrixUtilities.h:53-74), then the same from
 *                                                                        the exact-division build (must be equal)
 *   HRT_KAT_TRIANGLE  prim = c0, c1, c2 (Triangle ctor)         ray 7    8: hit, t, w0, w1, w2, normal (Triangle.h:77-126)
 *   HRT_KAT_AABB      prim = lo, hi                             ray 7    2: AABB::intersects (AABB.h:48-65), shipped gate
 *   HRT_KAT_SPHERE    prim = centre, radius, motion             ray 7    9: hit, t, theta, phi, normal, p.x, p.y (Sphere.h:91-132)
 *   HRT_KAT_QUAD      prim = v0, v1, v3, motion, glass          ray 7    8: hit, t, u, v, normal (Square.h:65-126), filter bit
 *   HRT_KAT_OPTICS    -                                         d, n, eta, cosine   8: reflect, refract, reflectance, gamma(|cosine|)
 *   HRT_KAT_NORMALIZE -                                         v        3: v / |v| (Vec3.h:46)
 *   HRT_KAT_HITWORD   -                                         kind, index, soup slot (u32 bit patterns)   4: the hit word of a
 *                     path record of the streaming kernel (kind | index, or kind | mesh | soup slot), then the kind, index and
 *                     soup slot read back from it (u32 bit patterns)
 *   HRT_KAT_DIV_KNOWN -                                         a, c     1: a / c by the shipped streaming builds' division by a known
 *                                                                        divisor (two FMAs; 1.f / c taken on the device, as their staging does)
 *   HRT_KAT_NORMALIZE_SHARED -                                  v        3: v / |v| with one reciprocal shared by the components
 *   HRT_KAT_QUAD_RCP  as HRT_KAT_QUAD                           ray 7    8: as HRT_KAT_QUAD, the quotients by |R| and |U| through their
 *                                                                        reciprocals (taken on the device) */
enum { HRT_KAT_CAMERA = 0, HRT_KAT_TRIANGLE = 1, HRT_KAT_AABB = 2, HRT_KAT_SPHERE = 3, HRT_KAT_QUAD = 4, HRT_KAT_OPTICS = 5,
       HRT_KAT_NORMALIZE = 6, HRT_KAT_HITWORD = 7, HRT_KAT_DIV_KNOWN = 8, HRT_KAT_NORMALIZE_SHARED = 9, HRT_KAT_QUAD_RCP = 10 };
HRT_API int hrt_debug_kat(uint32_t which, const hrt_camera *cam, const float *prim, const float *in, uint32_t n, float *out);

/* Cycle counters per kernel stage of the last launch; all zero unless libhrt.so was built with
 * -DHRT_STAMPS (diagnostic build, tools/variants.sh).  out: 16 values. */
HRT_API int hrt_debug_read_stamps(hrt_scene *scene, uint64_t out[16]);

/* Which build of the trace kernel a launch runs ("Builds and how one is chosen"): the library's own choice
 * function on plain values, so that the policy can be tested without a GPU and without hrt_init.  The scene's traits (tab_rows:
 * 16-byte rows of its per-object tables), the launch's tiles (after a tile list or batched views have set the count) and samples
 * per pixel, its flags, whether it has a tile list, its views (0 = not batched), and the value of the HRT_KERNEL environment
 * variable ("single", "dual", "stream"; NULL, "" or anything else = the default), which hrt_init parses with the same code.
 * Writes the kernel's name to name[cap] and returns HRT_OK, or returns the error the launch would (name = ""). */
typedef struct hrt_pick_input {
    uint32_t n_meshes, n_lights, n_spheres, tab_rows;
    uint32_t tiles, spp;
    uint32_t flags, has_list, n_views;
    const char *hrt_kernel;
} hrt_pick_input;
HRT_API int hrt_debug_pick_kernel(const hrt_pick_input *in, char *name, size_t cap);
/* The name of the build the scene's last trace launch ran ("" before any). */
HRT_API int hrt_debug_last_kernel(hrt_scene *scene, char *name, size_t cap);
/* The HIP resources the library holds at this moment, in every scene, history and multi handle and in calls under way:
 * out[0] device buffers, out[1] pinned host buffers, out[2] events, out[3] streams.  Each is counted where it is acquired and
 * where it is freed, so a handle's destroy call brings the numbers back to what they were before its creation.  Needs no hrt_init,
 * makes no HIP call and cannot fail. */
HRT_API void hrt_debug_live_resources(uint64_t out[4]);

/* Output stage of main.cpp:252-262: P3 ASCII with (int)(255*min(1,c)). */
/* The tree build's split search and partition on the GPU (a hrt_kd_builder_fn; `user` is ignored): level by level, every
 * candidate plane of every open node evaluated in parallel with the host builder's arithmetic and tie-breaking, so the
 * nodes -- and the flattened tree -- are identical to the host builder's (tests compare the arrays).  Exhaustive in the
 * candidates (references x candidates per node): meant for meshes up to a few hundred thousand triangles.  Needs hrt_init. */
HRT_API int hrt_kd_build_gpu(const hrt_kd_build_input *in, hrt_kd_build_output *out, void *user);

HRT_API int hrt_write_ppm(const char *path, const float *rgb, uint32_t w, uint32_t h);

/* ---- progressive rendering / resume (replaces the all-or-nothing sample loop main.cpp:188-195)
 * d_sum_tiles (device, hrt_tiles_owned()*HRT_TILE^2*3 floats, zeroed by the caller before the first call) holds
 * the running per-pixel SUMS of samples [0, first_sample); the call adds samples [first_sample, first_sample +
 * n_samples) in sample order.  Because a sample's random numbers depend only on (seed, pixel, sample index) and
 * the sum continues in the same order, k calls covering [0, N) leave exactly the bits one hrt_render_tiles of N
 * samples would have summed: a render can be previewed, stopped, checkpointed (copy the buffer) and resumed.
 * HRT_FLAG_GAMMA is ignored here; hrt_finalize_tiles applies it. */
HRT_API int hrt_render_accumulate(hrt_scene *scene, const hrt_camera *cam, uint32_t w, uint32_t h,
                          uint32_t first_sample, uint32_t n_samples, uint64_t seed, uint32_t flags,
                          uint32_t rank, uint32_t world, float *d_sum_tiles, void *stream);
/* sums -> pixel means (`image[i] /= nsamples`, main.cpp:195) and, with HRT_FLAG_GAMMA, gamma_correct
 * (main.cpp:196).  d_tiles may alias d_sum_tiles.  The result is what hrt_render_tiles(total_samples) writes. */
HRT_API int hrt_finalize_tiles(const float *d_sum_tiles, uint32_t n_tiles, uint32_t total_samples, uint32_t flags,
                       float *d_tiles, void *stream);
/* ---- adaptive sampling: per-tile sample counts set by a noise estimate ("render until clean")
 * Work is per HRT_TILE x HRT_TILE tile.  Round 0 adds samples [0, min_spp/2) to every tile, round 1 adds [min_spp/2, min_spp).
 * After every round from round 1 on, each tile rendered in it is judged: with S_old the sums over its n_old samples before the
 * round and S_new those over n_new samples after it, per in-image pixel in fp32
 *     A = S_old / (float)n_old,  B = S_new / (float)n_new,
 *     e = (|B.r - A.r| + |B.g - A.g| + |B.b - A.b|) / sqrtf(1e-4f + |B.r| + |B.g| + |B.b|)     (sums left to right)
 * and tile_err = max e over the tile's in-image pixels, where a pixel whose e is NaN (a mean that is inf or NaN) counts as 0: a
 * tile whose in-image pixels are all non-finite has tile_err 0.  The tile stays active while tile_err >= threshold and
 * n_new < max_spp; the next round adds min(n, max_spp - n) samples to every active tile (the count doubles, clipped at max_spp).  Rounds end when
 * no tile is active.  So every count lies in {min_spp * 2^k} u {max_spp}; threshold 0 gives every tile max_spp, +inf every
 * tile min_spp, and min_spp == max_spp is a uniform render.
 * CONTRACT: every tile of the result is bit-identical to the same tile of hrt_render at the count that tile was given (a
 * sample's random numbers depend only on (seed, pixel, sample), and the sums continue in sample order).  A tile's decision
 * reads only its own pixels, so counts and pixels are the same for any rank / world partition.
 * Parameters: min_spp even and >= 2, max_spp >= min_spp, threshold not NaN and not negative (+inf allowed).  They, the camera
 * and the output pointers are checked before the scene and the library state: a bad one returns HRT_ERR_INVALID and
 * hrt_last_error() names it. */
typedef struct hrt_adaptive {
    uint32_t min_spp, max_spp;
    float threshold;
} hrt_adaptive;
/* This rank's tiles (rank r of world: tiles r, r + world, ...), layout of hrt_render_tiles, into DEVICE memory: d_tiles receives
 * the pixel means (gamma-corrected with HRT_FLAG_GAMMA), d_tile_spp one uint32 count per owned tile.  Runs on `stream` (a
 * hipStream_t, NULL = the default stream) and synchronises it once per round: one 4-byte read-back (how many tiles are still
 * active) sizes the next launch.  Every trace launch is checked (hrt_check_last_launch); a kernel that gave up ends the call
 * with HRT_ERR_DEVICE.  The rounds' scratch (compact sums, tile lists, counter) lives in the hrt_scene. */
HRT_API int hrt_render_adaptive_tiles(hrt_scene *scene, const hrt_camera *cam, uint32_t w, uint32_t h, const hrt_adaptive *params,
                                      uint64_t seed, uint32_t flags, uint32_t rank, uint32_t world, float *d_tiles,
                                      uint32_t *d_tile_spp, void *stream);
/* The whole frame on the scene's device into a HOST buffer out_rgb[h*w*3], as hrt_render.  out_tile_spp (host, may be NULL):
 * tiles_y * tiles_x counts, row-major.  stats (may be NULL): kernel_ms = the trace kernels' time summed over all rounds,
 * samples = sum over in-image pixels of their tile's count. */
HRT_API int hrt_render_adaptive(hrt_scene *scene, const hrt_camera *cam, uint32_t w, uint32_t h, const hrt_adaptive *params,
                                uint64_t seed, uint32_t flags, float *out_rgb, uint32_t *out_tile_spp, hrt_stats *stats);

/* ---- denoising: first-hit feature buffers and an edge-avoiding a-trous wavelet filter (Dammertz et al., HPG 2010)
 * FEATURES, per pixel (x, y) (pixel index y*w + x) and per sample s in [first_sample, first_sample + n_samples): the camera ray of
 * that sample exactly as the trace kernels draw it (the RNG stream (seed, pixel, s): u, v, time, then the camera), its closest hit
 * and the shading of that hit -- the device functions hrt_render_aov uses.  So pixel, sample and seed give the ray and first hit of
 * that sample in hrt_render.  n_samples == 0: one ray through the pixel centre at time 0 (hrt_render_aov's rays: albedo, normal,
 * emission and depth are then its outputs bit for bit).  HRT_FEATURE_FLOATS floats per pixel, row-major:
 *     albedo rgb, shading normal xyz, emission rgb, depth (the hit's t), coverage (fraction of samples that hit), 0
 * each = (sum over the samples in sample order, in fp32, starting from +0) / (float)n (n = 1 for n_samples == 0); a miss adds 0. */
#define HRT_FEATURE_FLOATS 12
/* d_features: device, h*w*HRT_FEATURE_FLOATS floats.  Runs on `stream`, asynchronously, with a camera block of its own (a trace
 * launch on another stream cannot see it); feature launches of one scene on different streams are ordered. */
HRT_API int hrt_render_features(hrt_scene *scene, const hrt_camera *cam, uint32_t w, uint32_t h, uint32_t first_sample, uint32_t n_samples, uint64_t seed, float *d_features, void *stream);
/* THE FILTER.  Input: c = linear pixel means (h*w*3) and the features above (a = albedo, n = normal, e = emission, z = depth).
 * All arithmetic is fp32 without fused multiply-add, in the order written; tests/denoise_ref.py states the same rule in numpy.
 * 1. Demodulate: d_k = a_k if a_k > 0 else 1,  x_k = (c_k - e_k / 6) / d_k.  A first hit contributes (direct + E + a * incoming) / 6
 *    to a sample and `direct` carries the albedo as a factor for every material type (diffuse, glass, mirror: shade() sets one
 *    albedo, direct_light multiplies each light term by it, the throughput is multiplied by it), so x is exact for a pixel covered
 *    by one surface.  Misses (a = 0, e = 0) and albedo-0 emitters are filtered in colour space (d = 1).
 *    A pixel is INVALID when a component of x or of its albedo, normal, emission or depth is not finite; its x becomes NaN.
 * 2. Iterate, i = 0 .. iterations-1, step s = 2^i:  y_p = (sum_q w_pq x_q) / (sum_q w_pq)  over the 5x5 taps q = p + s*(j, k),
 *    rows k = -2..2 outer, columns j = -2..2 inner; taps outside the image and taps whose x is not finite are skipped.  An invalid
 *    pixel keeps y_p = x_p (NaN).  The centre tap has w = h_0 h_0; any other tap
 *        w_pq = (h_j h_k) * expf(-E),  E = ((T(|x_p - x_q|^2, (sc_i)^2) + T(|n_p - n_q|^2, sn^2)) + T(|a_p - a_q|^2, sa^2)) + T((z_p - z_q)^2, (sz * max(max(z_p, z_q), 1e-3))^2)
 *    with h = (1, 4, 6, 4, 1) / 16, sc_i = sigma_color * 2^-i (the colour term tightens every iteration), |v|^2 = (v0 v0 + v1 v1) + v2 v2,
 *    and T(num, den) = 0 if num == 0 or den == +inf, else num / den (so sigma = +inf switches a term off).  The sums run in tap order:
 *    sum_w += w, sum_x += w * x_q per channel.
 * 3. Remodulate: r_k = d_k * y_k + e_k / 6.  A pixel with a non-finite component of r is written as its input c instead (invalid
 *    pixels therefore pass through unchanged).  With HRT_FLAG_GAMMA every value v then becomes (float)pow((double)v, 1/2.2), the
 *    arithmetic of hrt_finalize_tiles.  A finite input never gives a non-finite linear output.
 * Parameters: iterations 1..8, every sigma > 0 and not NaN (+inf allowed), w and h positive, flags HRT_FLAG_GAMMA or 0, no NULL
 * pointer.  They are checked before any device call: a bad one returns HRT_ERR_INVALID and hrt_last_error() names it. */
typedef struct hrt_denoise_params {
    uint32_t iterations;                                          /* 1..8; step of iteration i = 2^i pixels */
    float sigma_color, sigma_normal, sigma_albedo, sigma_depth;   /* > 0; +inf switches a term off       */
} hrt_denoise_params;
/* Bytes of d_scratch hrt_denoise needs for a w x h frame (the packed guides and two ping-pong colour buffers, 64 per pixel). */
HRT_API size_t hrt_denoise_scratch_bytes(uint32_t w, uint32_t h);
/* Device pointers, asynchronous on `stream`.  d_color: h*w*3 linear means; d_features: as hrt_render_features writes them;
 * d_out: h*w*3 (must not alias the inputs or the scratch). */
HRT_API int hrt_denoise(const float *d_color, const float *d_features, uint32_t w, uint32_t h, const hrt_denoise_params *p, uint32_t flags, void *d_scratch, float *d_out, void *stream);
/* The whole frame on the scene's device into a HOST buffer out_rgb[h*w*3]: hrt_render's frame at spp samples, linear (by the kernel
 * form hrt_render picks; the kernel-form flags apply), checked with hrt_check_last_launch, the features of samples [0, feature_spp)
 * (feature_spp <= spp; 0 = pixel centres), then hrt_denoise with HRT_FLAG_GAMMA as given in flags.  The frame never leaves the
 * device; the scratch lives in the hrt_scene, grown on demand.  The result is bit-identical to hrt_denoise(hrt_render(...) without
 * gamma, hrt_render_features(0, feature_spp)).  stats (may be NULL): kernel_ms = the trace kernel's time, as hrt_render. */
HRT_API int hrt_render_denoised(hrt_scene *scene, const hrt_camera *cam, uint32_t w, uint32_t h, uint32_t spp, uint32_t feature_spp, uint64_t seed, uint32_t flags, const hrt_denoise_params *p, float *out_rgb, hrt_stats *stats);

/* ---- variance-guided denoising: the filter above with a colour width PER PAIR OF PIXELS, the estimated variance of the
 * difference of the two pixels' own means (the spatial half of SVGF, Schied et al., HPG 2017).  Where the frame is still noisy the colour term is wide, where it has
 * converged it is narrow and the detail survives.  hrt_denoise and hrt_render_denoised are unchanged.
 * Input: c = linear means over all N samples, c_half = linear means over the first N/2 samples of the same render (N even), and the
 * features of hrt_render_features.  All arithmetic is fp32 without fused multiply-add, in the order written;
 * tests/denoise_var_ref.py states the same rule in numpy.  T, h, |v|^2, d, the tap order and the skipping of taps are those of THE
 * FILTER above; G_pq = (T(|n_p - n_q|^2, sn^2) + T(|a_p - a_q|^2, sa^2)) + T((z_p - z_q)^2, (sz * max(max(z_p, z_q), 1e-3))^2) are its
 * guide terms.
 * 1. Demodulate both frames with step 1 above (e_k / 6 is computed once per channel): x from c, x_half from c_half.  A pixel is
 *    INVALID when it is invalid for either frame; its x becomes NaN.  Variance of the mean, summed over the channels:
 *    delta = x - x_half (half the difference of the two half means), v = (delta_0 delta_0 + delta_1 delta_1) + delta_2 delta_2;
 *    v = 0 on an invalid pixel and where that sum is not finite.
 * 2. Prefilter v alone, passes i = 0 .. prefilter-1 at step 2^i:  v_p <- (sum_q w_pq v_q) / (sum_q w_pq)  with w = h_0 h_0 at the
 *    centre and w_pq = (h_j h_k) * expf(-G_pq) elsewhere; sum_w += w, sum_v += w * v_q.  An invalid pixel keeps its v.
 * 3. Iterate, i = 0 .. iterations-1, step 2^i, as step 2 above with
 *        w_pq = (h_j h_k) * expf(-E),  E = T(|x_p - x_q|^2, D_pq) + G_pq,
 *        D_pq = +inf if sigma_variance == +inf, else (sigma_variance * sigma_variance) * ((v_p + v_q) + variance_floor)
 *    (the width is the variance of the difference of the two means, the same for both pixels of a pair, so a bright outlier hands
 *    on what it loses; it is not tightened over the iterations: the variance shrinks by itself), and the
 *    variance carried along:  v_p <- (sum_q (w_pq w_pq) v_q) / (sum_w sum_w), the centre tap included with w = h_0 h_0;
 *    sum_v += (w * w) * v_q in tap order beside sum_w and sum_x.  An invalid pixel keeps x (NaN) and v (0).
 * 4. Remodulate, fall back to the input pixel c, gamma: step 3 above, unchanged.  d_variance_out, if wanted, receives the final v
 *    (h*w floats, in demodulated units): an error map of the result.
 * Parameters: iterations 1..8, prefilter 0..4, every sigma > 0 and not NaN (+inf switches its term off), variance_floor finite and
 * >= 0, w and h positive, flags HRT_FLAG_GAMMA or 0; spp even and >= 2, feature_spp <= spp.  They are checked before any device call:
 * a bad one returns HRT_ERR_INVALID and hrt_last_error() names it. */
typedef struct hrt_denoise_var_params {
    uint32_t iterations;                                           /* 1..8; step of iteration i = 2^i pixels            */
    uint32_t prefilter;                                            /* 0..4 passes over the variance before the iterations */
    float sigma_variance, sigma_normal, sigma_albedo, sigma_depth; /* > 0; +inf switches a term off                       */
    float variance_floor;                                          /* >= 0, added to v_p + v_q in the colour width      */
} hrt_denoise_var_params;
/* Bytes of d_scratch hrt_denoise_var needs for a w x h frame (the packed guides and two ping-pong {x, v} buffers, 64 per pixel). */
HRT_API size_t hrt_denoise_var_scratch_bytes(uint32_t w, uint32_t h);
/* Device pointers, asynchronous on `stream`.  d_color, d_color_half: h*w*3 linear means; d_features: as hrt_render_features writes
 * them; d_out: h*w*3; d_variance_out: h*w, may be NULL (neither may alias the inputs or the scratch). */
HRT_API int hrt_denoise_var(const float *d_color, const float *d_color_half, const float *d_features, uint32_t w, uint32_t h, const hrt_denoise_var_params *p, uint32_t flags, void *d_scratch, float *d_out, float *d_variance_out, void *stream);
/* The whole frame on the scene's device into HOST buffers out_rgb[h*w*3] and out_variance[h*w] (may be NULL): samples [0, spp/2)
 * with hrt_render_accumulate, a copy of those sums, samples [spp/2, spp) on top, both finalised without gamma (every launch checked
 * with hrt_check_last_launch), the features of samples [0, feature_spp), then hrt_denoise_var with HRT_FLAG_GAMMA as given in flags
 * (the kernel-form flags apply).  Nothing but the result leaves the device.  The result is bit-identical to hrt_denoise_var(
 * hrt_render(spp), hrt_render(spp/2), hrt_render_features(0, feature_spp)), both renders without gamma.  stats (may be NULL):
 * kernel_ms = the two trace launches' time. */
HRT_API int hrt_render_denoised_var(hrt_scene *scene, const hrt_camera *cam, uint32_t w, uint32_t h, uint32_t spp, uint32_t feature_spp, uint64_t seed, uint32_t flags, const hrt_denoise_var_params *p, float *out_rgb, float *out_variance, hrt_stats *stats);

/* ---- temporal accumulation: the previous accumulated frame reprojected under a moved camera and blended with the current one
 * (the temporal half of SVGF, Schied et al., HPG 2017).  The frame c and its first-half frame c_half are accumulated with the same
 * taps and the same weights, so x - x_half of the accumulated pair is the weighted sum of the frames' own differences, and its
 * square estimates the variance of the accumulated mean: the accumulated pair can be handed to the unchanged hrt_denoise_var, whose
 * colour width then narrows by itself as history grows.  No existing entry point changes.
 * Input: c (and c_half) = linear means of the current frame, its features (a, n, e, z, cov as hrt_render_features writes them) and
 * camera; the previous call's outputs (colour, half colour, history), the features they were accumulated with and that frame's
 * camera.  All arithmetic is fp32 without fused multiply-add, in the order written; tests/temporal_ref.py states the same rule in
 * numpy.  d, |v|^2 and "finite" are those of THE FILTER above.  For pixel p = (x, y):
 * 1. Demodulate c (and c_half) with step 1 of THE FILTER: x_p (and xh_p).  p is a RESTART pixel if it is invalid under that rule
 *    (for either frame), if cov == 0 (no sample hit anything), if no previous frame was given, or if a later step finds no usable
 *    history.  A restart pixel writes out = c, out_half = c_half, history_out = 1.
 * 2. World point: zbar = z / cov;  r = camera_ray(cam, (x + 0.5) / w, (y + 0.5) / h, 0), the device function of the trace kernels
 *    (what hrt_debug_kat(HRT_KAT_CAMERA) returns for that u, v);  P_k = r.o_k + zbar * r.d_k.
 * 3. Project into the previous camera: s = P - prev_cam->eye;  xc = (s0 R0 + s1 R1) + s2 R2 with R = prev_cam->right, yc and zc the
 *    same with up and forward.  !(zc > 0): restart.  With cot = cos(rad) / sin(rad), rad = fovy_deg / 2 * pi / 180 in fp64 on the host
 *    (the projection hrt_render builds), kx = (float)(cot / aspect), ky = (float)cot of prev_cam:
 *        px = (((kx * xc) / zc + 1) * 0.5f) * (float)w - 0.5f,   py = ((1 - (ky * yc) / zc) * 0.5f) * (float)h - 0.5f,
 *        zexp = sqrtf((s0 s0 + s1 s1) + s2 s2)            (the depth the previous frame would have recorded for P).
 *    STATIC CAMERA: when memcmp(cam, prev_cam, sizeof(hrt_camera)) == 0, px = x, py = y, zexp = zbar instead: a still camera
 *    accumulates pixel onto pixel, without resampling blur.
 * 4. Taps: ix = floorf(px), iy = floorf(py), fx = px - ix, fy = py - iy; the taps q are (ix, iy), (ix+1, iy), (ix, iy+1),
 *    (ix+1, iy+1) in that order with weights (1-fx)(1-fy), fx(1-fy), (1-fx)fy, fx fy.  A tap is USED only if it lies inside the
 *    image, history_prev[q] >= 1, q's previous features 0..10 are finite with cov_q > 0, q's previous colour(s) demodulated with
 *    q's previous features are finite, and
 *        |zexp - z_q / cov_q| <= depth_tol * fmaxf(zexp, 1e-3f),   |n_p - n_q|^2 <= normal_tol,   |a_p - a_q|^2 <= albedo_tol
 *    (a tolerance of +inf passes its test always).  Sums in tap order over the used taps: sw += w, sx += w * x_q per channel,
 *    sxh += w * xh_q, sn += w * history_prev[q].  !(sw > 0): restart.
 * 5. Blend: n_new = fminf(sn / sw + 1, max_history), alpha = fmaxf(1 / n_new, alpha_min), xhist = sx / sw,
 *    y = xhist + alpha * (x_p - xhist), and the same for the half frame with the same alpha.  Remodulate with the CURRENT features as
 *    step 3 of THE FILTER: r_k = d_k * y_k + e_k / 6.  A non-finite component of r (of either frame) writes the input pixel and
 *    history_out = 1; otherwise out = r, out_half = r_half, history_out = n_new.
 * Colours are h*w*3, features h*w*HRT_FEATURE_FLOATS, history h*w floats, all device pointers; asynchronous on `stream`, no scene:
 * the call runs on the calling thread's current device, like hrt_camera_rays.  prev_cam and the four d_prev_* pointers are all given
 * or all NULL (NULL: the first frame, every pixel restarts); d_prev_color_half is given iff d_color_half is, d_out_half iff
 * d_color_half is.  Outputs must not alias any input.
 * Checked before any device call, HRT_ERR_INVALID with hrt_last_error() naming hrt_temporal_accumulate and the culprit: NULL or
 * inconsistent pointers, w or h zero or w*h over the denoisers' frame limit, alpha_min outside (0, 1] or NaN, max_history < 1, NaN or
 * infinite, a tolerance <= 0 or NaN, a camera hrt_render refuses. */
typedef struct hrt_temporal_params {
    float alpha_min;      /* (0, 1]: floor of the blend weight of the current frame; 1 = no history is used        */
    float max_history;    /* >= 1, finite: history length saturates here                                            */
    float depth_tol;      /* > 0, +inf switches the test off: relative depth disagreement a tap may have            */
    float normal_tol;     /* > 0, +inf off: |n_p - n_q|^2 a tap may have                                            */
    float albedo_tol;     /* > 0, +inf off: |a_p - a_q|^2 a tap may have                                            */
} hrt_temporal_params;
HRT_API int hrt_temporal_accumulate(const hrt_camera *cam, const hrt_camera *prev_cam, uint32_t w, uint32_t h,
    const float *d_color, const float *d_color_half /* may be NULL */, const float *d_features,
    const float *d_prev_color, const float *d_prev_color_half, const float *d_prev_features, const float *d_prev_history,
    const hrt_temporal_params *p,
    float *d_out, float *d_out_half /* NULL iff d_color_half is */, float *d_history_out, void *stream);
/* THE FRAME LOOP.  An hrt_history holds, on the scene's device, what one frame hands to the next: the accumulated pair, the
 * features it was accumulated with, the history lengths, the camera and the frame size.  hrt_render_temporal renders one frame into
 * the HOST buffer out_rgb[h*w*3]: the two half renders and the features exactly as hrt_render_denoised_var makes them (spp even and
 * >= 2, feature_spp <= spp, every launch checked), hrt_temporal_accumulate against the stored state (none after create or reset, or
 * when w or h differ from the stored frame's: then every pixel restarts), the outputs stored as the new state (two buffer sets swap
 * roles, nothing is copied); then with dp hrt_denoise_var on the accumulated pair and the current features, HRT_FLAG_GAMMA as given in
 * flags, or without dp the accumulated frame itself with hrt_finalize_tiles' gamma.  The filtered frame is never fed back: only the
 * accumulated pair is history.  out_history (host, h*w, may be NULL) receives the history lengths.
 * CONTRACT: the result is bit-identical to composing hrt_render(spp), hrt_render(spp / 2), hrt_render_features(0, feature_spp),
 * hrt_temporal_accumulate and hrt_denoise_var by hand.  The caller passes a DIFFERENT seed for every frame: with the same seed a
 * still camera renders the same samples again and gains nothing.  A history belongs to the scene it was created for. */
typedef struct hrt_history hrt_history;
HRT_API int hrt_history_create(hrt_scene *scene, hrt_history **out);
HRT_API void hrt_history_reset(hrt_history *hist);      /* the next frame restarts everywhere */
/* Frees the history's device buffers, also when called after hrt_shutdown (as hrt_scene_destroy frees a scene's; before the
 * buffers owned themselves, a history destroyed after hrt_shutdown left its eight buffers behind). */
HRT_API void hrt_history_destroy(hrt_history *hist);
HRT_API int hrt_render_temporal(hrt_scene *scene, hrt_history *hist, const hrt_camera *cam, uint32_t w, uint32_t h,
                                uint32_t spp, uint32_t feature_spp, uint64_t seed, uint32_t flags,
                                const hrt_temporal_params *tp, const hrt_denoise_var_params *dp /* NULL: no spatial filter */,
                                float *out_rgb, float *out_history /* host h*w, may be NULL */, hrt_stats *stats);

/* ---- ray queries: the scene traced with the caller's own rays (picking, visibility, baking, hit buffers for other code)
 * RAYS: n records of 8 floats (32 bytes, the array 16-byte aligned) {o.x, o.y, o.z, time, d.x, d.y, d.z, tmax}, device memory.
 * CLOSEST: Scene::computeIntersection (Scene.h:202-230) on the ray exactly as given -- no normalisation unless HRT_RAYS_NORMALIZE,
 * `time` places the moving objects (motion blur) -- and the hit is reported only if t < tmax (tmax = +inf: the reference's
 * unbounded query).  Output, 4 x 32 bits per ray: {t (float), kind (u32: 0 miss, 1 sphere, 2 square, 3 mesh), index (u32: the
 * object), prim (u32: the reference triangle id of a mesh hit, the id hrt_render_aov reports; 0xFFFFFFFF otherwise)}.  A miss is
 * {0, 0, 0xFFFFFFFF, 0xFFFFFFFF}.
 * SHADE: 16 x 32 bits per ray: the CLOSEST record, {n.xyz, transparency}, {albedo.rgb, index_medium}, {emission.rgb, material type
 * (u32)} -- the values shade() gives, hence those of hrt_render_aov and hrt_render_features for the same ray.  On a miss every field
 * after the CLOSEST record is 0.
 * OCCLUDED: one u32 per ray, 1 if some object's own hit (the value CLOSEST compares for it) has EPSILON <= t < tmax, else 0:
 * Scene::computeShadow (Scene.h:235-255) with every transparency taken as 0, so deterministic, no random numbers.  It equals
 * (CLOSEST.kind != 0).  An object ends the query only as a whole: a mesh whose nearest triangle has 0 <= t < EPSILON hides its
 * farther triangles from that ray, as in the closest hit.
 * DEGENERATE rays -- a component of o, d or time not finite, d == 0, tmax NaN or <= 0, or with HRT_RAYS_NORMALIZE a normalised d
 * that is not finite or is 0 -- are not traced: the miss record, 0 for OCCLUDED.
 * Flags: HRT_FLAG_EXACT_ONLY (proof build), HRT_FLAG_MESH_BRUTE (with EXACT_ONLY), HRT_FLAG_NO_LDS_TREE (accepted; queries read the
 * tree from global memory anyway, DESIGN.md section 5 "Ray queries"), HRT_RAYS_NORMALIZE (apply
 * the Ray constructor's normalisation, Line.h:13-16, to d first: then the records equal those of the normalised rays).  All give
 * the same records.  Any other bit is refused.
 * Checked before the scene and the library state, HRT_ERR_INVALID with hrt_last_error() naming the culprit: mode, flags, NULL or
 * misaligned pointers when n > 0 (d_rays 16 bytes; d_out 16 bytes, 4 for OCCLUDED), n > 2^31 - 1; then a NULL scene.  n == 0
 * returns HRT_OK and launches nothing.
 * CONCURRENCY: asynchronous on `stream` (a hipStream_t, NULL = the default stream).  The call touches none of the per-launch
 * state of the scene (work-queue head, path pool, camera blocks): a query may run on another stream at the same time as a render
 * of the same scene, and queries of one scene on several streams may overlap. */
enum { HRT_QUERY_CLOSEST = 0, HRT_QUERY_SHADE = 1, HRT_QUERY_OCCLUDED = 2 };
#define HRT_RAYS_NORMALIZE 256u
#define HRT_RAY_FLOATS 8
HRT_API int hrt_trace_rays(hrt_scene *scene, const float *d_rays, uint32_t n, uint32_t mode, uint32_t flags, void *d_out, void *stream);

/* ---- radiance queries: the path-traced colour of the caller's own rays (baking, light probes, panoramas, other camera models)
 * RAYS: the records of hrt_trace_rays ({o, time, d, tmax}, device memory, 16-byte aligned); tmax is not read.  Ray i has the key
 * k = d_keys ? d_keys[i] : i.  For each sample s in [first_sample, first_sample + n_samples), in that order, one path runs: RNG
 * stream (seed, k, s) from draw 3 on (draws 0..2 are the camera's u, v, time), first segment the caller's ray as given (`time`,
 * the same for every sample, places the moving objects), then exactly the render's integrator: HRT_MAXBOUNCES bounces, the sky
 * (Scene::skyboxTexture with the bounces left), direct light with soft shadows, scatter, the exact pruning of the render, and
 * sum += radiance / 6.
 * OUTPUT: 3 floats per ray at d_out[3i .. 3i+2]: sum / (float)n_samples; with HRT_RADIANCE_ACCUMULATE d_out holds the running
 * sums of samples [0, first_sample) on entry, the call adds its samples in order and stores the raw sums (as
 * hrt_render_accumulate).
 * DEGENERATE rays (the rule of hrt_trace_rays without tmax: a component of o, d or time not finite, d == 0, or with
 * HRT_RAYS_NORMALIZE a normalised d that is not finite or is 0) add nothing: 0 in mean mode, their sums left as they are under
 * HRT_RADIANCE_ACCUMULATE.
 * CONTRACT: take the records hrt_camera_rays(cam, w, h, s, seed) writes and trace them with first_sample = s, n_samples = 1,
 * d_keys = NULL for s = 0..S-1; the outputs summed in sample order in fp32 and divided by (float)S are hrt_render(cam, w, h, S,
 * seed) without HRT_FLAG_GAMMA, bit for bit, for every scene and every kernel form.
 * Flags: HRT_FLAG_EXACT_ONLY (proof build), HRT_FLAG_MESH_BRUTE (with EXACT_ONLY), HRT_FLAG_NO_LDS_TREE (accepted; radiance queries
 * read the tree from global memory anyway, DESIGN.md section 5 "Radiance queries"), HRT_RAYS_NORMALIZE, HRT_RADIANCE_ACCUMULATE.  The
 * first three give the same values.  Any other bit is refused.
 * Checked before the scene and the library state, HRT_ERR_INVALID with hrt_last_error() naming the culprit: flags, NULL or
 * misaligned pointers when n > 0 (d_rays 16 bytes; d_keys, if given, and d_out 4 bytes), n > 2^31 - 1, n_samples == 0,
 * first_sample + n_samples > 2^32 (sample indices do not wrap); then a NULL scene.  n == 0 returns HRT_OK and launches nothing.
 * CONCURRENCY: as hrt_trace_rays -- asynchronous on `stream`, no per-launch state of the scene is touched, so radiance queries may
 * overlap a render of the same scene on another stream. */
#define HRT_RADIANCE_ACCUMULATE 512u
HRT_API int hrt_trace_radiance(hrt_scene *scene, const float *d_rays, const uint32_t *d_keys, uint32_t n, uint32_t first_sample,
                               uint32_t n_samples, uint64_t seed, uint32_t flags, float *d_out, void *stream);
/* The camera rays of sample `sample` of a w x h frame as ray records (device, 16-byte aligned, w*h records, pixel y*w + x):
 * u = (x + draw0) / w, v = (y + draw1) / h, time = draw2 of stream (seed, y*w + x, sample); o and d are the render's camera ray
 * (d normalised twice, as the reference); tmax = +inf.  No scene: it runs on the calling thread's current device, asynchronously
 * on `stream`, and the camera block travels as a kernel argument.  Refused (HRT_ERR_INVALID): a NULL cam, a camera hrt_render
 * refuses, w or h zero, w*h > 2^31 - 1, d_rays NULL or misaligned (checked in that order, before the library state). */
HRT_API int hrt_camera_rays(const hrt_camera *cam, uint32_t w, uint32_t h, uint32_t sample, uint64_t seed, float *d_rays, void *stream);

/* ---- Batched views: many cameras of one scene, every one a w x h frame of spp samples, in ONE trace launch.
 * N views make one work queue of N x hrt_tiles_total(w, h) items (item j: tile j % tiles of view j / tiles), so the samples of
 * all views are spread over all workgroups: small frames, which do not fill the device one at a time, do so together.
 * CONTRACT: frame v is bit-identical to hrt_render(scene, &views[v].cam, w, h, spp, views[v].seed, flags), for every scene, every
 * n_views and every permitted flag combination.  The random numbers of a sample depend only on (seed of its view, pixel y*w + x
 * inside its view, sample).
 * FLAGS: HRT_FLAG_GAMMA, HRT_FLAG_NO_LDS_TREE, HRT_FLAG_WAVE_KERNEL, HRT_FLAG_STREAM_KERNEL, HRT_FLAG_NO_SHADOW_CULL.  Refused by
 * name: HRT_FLAG_DUAL_KERNEL, HRT_FLAG_EXACT_ONLY, HRT_FLAG_MESH_BRUTE (no batched builds of those kernel forms); any other bit is
 * refused.  Without a forced form the kernel form is hrt_render_tiles' choice for the TOTAL tile count, which may differ from the
 * form one view alone would get; all forms give the same pixels.
 * hrt_render_views_device: d_frames (device) receives n_views * h * w * 3 floats, view-major, each view row-major as
 * hrt_render's; asynchronous on `stream` (call hrt_check_last_launch before the frames are used).  `views` may be freed when the
 * call returns.  The tile sums and the per-view blocks are scratch of the scene.
 * hrt_render_views: the same into a HOST buffer, blocking, checked with hrt_check_last_launch; stats as hrt_render
 * (samples = n_views * w * h * spp).
 * LIMIT: n_views x hrt_tiles_total(w, h) <= HRT_VIEWS_MAX_TILES, so that a work-queue item (a tile, shifted left by up to 2 bits
 * when tiles are split into row bands) and the float index of the tile sums (192 per tile) fit 32 bits.
 * Checked in this order before the scene and the library state, HRT_ERR_INVALID with hrt_last_error() naming the entry point and
 * the culprit: flags; (n_views == 0 returns HRT_OK here and launches nothing;) views NULL; w, h, spp as hrt_render checks them;
 * every camera as hrt_render checks it, with the index of the offending view; the output pointer NULL or not 4-byte aligned;
 * the limit above; then a NULL scene. */
typedef struct hrt_view {
    hrt_camera cam;
    uint64_t seed;
} hrt_view;
#define HRT_VIEWS_MAX_TILES (1u << 24)
HRT_API int hrt_render_views_device(hrt_scene *scene, const hrt_view *views, uint32_t n_views, uint32_t w, uint32_t h,
                                    uint32_t spp, uint32_t flags, float *d_frames, void *stream);
HRT_API int hrt_render_views(hrt_scene *scene, const hrt_view *views, uint32_t n_views, uint32_t w, uint32_t h,
                             uint32_t spp, uint32_t flags, float *out_rgb, hrt_stats *stats /* may be NULL */);

/* ---- Lens cameras: depth of field, orthographic, equirectangular and fisheye frames through the unchanged integrator.
 * A lens is a camera hrt_render accepts plus a projection; hrt_camera itself and every entry point that takes one stay as they are.
 * THE RULE (the ray of sample s of pixel p = y*w + x; tests/lens_ref.py states it again in NumPy):
 *   Draws: g0, g1, g2 are draws 0, 1, 2 of stream (seed, p, s); u = (x + g0)/w, v = (y + g1)/h, time = g2, exactly as the render's
 *   camera sample.  R, U, F, E are the camera's right, up, forward and eye as given.  All arithmetic is fp32 without fused
 *   multiply-add, in the order written; sqrtf, sinf, cosf are the device's; normalize is the trace path's own (divide by the length).
 *   PERSPECTIVE: r = the render's camera ray for (u, v, time).  aperture_radius == 0: the ray is r, untouched -- the record is
 *     hrt_camera_rays' bit for bit.  Otherwise l0, l1 are draws HRT_LENS_DRAW and HRT_LENS_DRAW + 1 of the same stream (the
 *     generator is counter-based; a path uses draws 3 onward and never comes near 2^31):
 *       rad = aperture_radius * sqrtf(l0), phi = 6.2831855f * l1, a = rad * cosf(phi), b = rad * sinf(phi)
 *       c = (d0 F0 + d1 F1) + d2 F2 with d = r.d; !(c > 0) makes a degenerate sample
 *       tf = focus_distance / c, P = r.o + tf * r.d, O = r.o + (a * R + b * U); the ray is {O, normalize(P - O), time}
 *     so every ray of a pixel sample passes through the point its pinhole ray has at depth focus_distance along forward.
 *   ORTHOGRAPHIC: sx = (2u - 1) * ((0.5f * extent) * aspect), sy = (1 - 2v) * (0.5f * extent); O = E + (sx * R + sy * U),
 *     d = normalize(F).
 *   EQUIRECT (the frame spans 360 x 180 degrees, its centre looks along F): phi = (2u - 1) * 3.1415927f,
 *     th = (0.5f - v) * 3.1415927f; d = normalize(((cosf(th) * sinf(phi)) * R + sinf(th) * U) + (cosf(th) * cosf(phi)) * F), O = E.
 *   FISHEYE (equidistant, the image circle inscribed in the frame height): qx = (2u - 1) * aspect, qy = 1 - 2v,
 *     rr = sqrtf(qx qx + qy qy); rr > 1 makes a degenerate sample; th = rr * (extent * 0.5f * (3.1415927f / 180.f)); rr == 0:
 *     d = normalize(F), otherwise k = sinf(th) / rr, d = normalize(((k * qx) * R + (k * qy) * U) + cosf(th) * F); O = E.
 *   A DEGENERATE sample is written by hrt_lens_rays as {E, time, 0, 0, 0, +inf}: d == 0 is the query layer's own rule for "not
 *   traced".  It adds nothing to a pixel and still counts in the divisor.
 * hrt_lens_rays: the sibling of hrt_camera_rays -- same record layout, no scene, the calling thread's current device, asynchronous on
 * `stream`.  Checked in this order before the library state (HRT_ERR_INVALID, hrt_last_error() naming the entry point and the
 * field): lens NULL; the camera, as hrt_render checks it; projection; aperture_radius; focus_distance; extent (each against the
 * comments of hrt_lens); the frame, as hrt_camera_rays checks it; d_rays NULL or misaligned.
 * hrt_render_lens_device: the frame without a ray buffer.  d_frame (device, h*w*3 floats, row-major) receives the mean over samples
 * [first_sample, first_sample + n_samples); with HRT_RADIANCE_ACCUMULATE it holds running sums, exactly as hrt_trace_radiance's
 * output does.  Asynchronous on `stream`; touches none of the scene's per-launch state, so it may overlap a render of the same
 * scene.  Flags: HRT_FLAG_EXACT_ONLY, HRT_FLAG_MESH_BRUTE (with EXACT_ONLY), HRT_FLAG_NO_LDS_TREE, HRT_RADIANCE_ACCUMULATE,
 * HRT_FLAG_GAMMA (hrt_finalize_tiles' arithmetic on the means; refused together with ACCUMULATE).  Any other bit is refused by name;
 * that includes the kernel-form flags, since there is one form.  Checked in this order: flags; the lens checks above; the frame;
 * n_samples == 0; first_sample + n_samples > 2^32; d_frame NULL or not 4-byte aligned; then a NULL scene.
 * CONTRACT A: bit-identical to composing, for s in order, hrt_lens_rays(s) and hrt_trace_radiance(first_sample = s, n_samples = 1,
 * d_keys = NULL), summed in fp32 and divided by (float)n_samples -- for every projection and flag set.
 * CONTRACT B: PERSPECTIVE with aperture_radius == 0 is bit-identical to hrt_render(&lens->cam, ...) with the same gamma flag, under
 * every kernel form of hrt_render.
 * hrt_render_lens: the same into a HOST buffer, blocking, samples [0, spp); stats as hrt_render (kernel_ms from events, samples =
 * w*h*spp).  HRT_RADIANCE_ACCUMULATE is refused (the sums live on the device).
 * hrt_render_lens_features: hrt_render_features with the lens in place of the camera -- same layout and sums -- so that a
 * depth-of-field or panorama frame can go into the unchanged hrt_denoise / hrt_denoise_var with guides that saw what the frame saw.
 * n_samples == 0 is the pixel centre u = (x + .5)/w, v = (y + .5)/h at time 0 with l0 = l1 = 0.  A degenerate sample counts as a
 * miss.  With PERSPECTIVE and aperture 0 it equals hrt_render_features bit for bit; with any other lens its hits are those of
 * hrt_trace_rays(HRT_QUERY_SHADE) on the records of hrt_lens_rays.  Asynchronous on `stream`; the lens travels as a kernel argument,
 * so unlike hrt_render_features the call takes no part in the ordering of the scene's feature launches.
 * Not lens-aware (DESIGN.md section 5 "Lens cameras"): the streaming kernel, temporal reprojection, the multi-GPU paths.  Adaptive
 * sampling under a lens is hrt_render_lens_adaptive further below.  Many lens frames in one launch are hrt_render_lens_views below: a batch through the lens kernels, not through
 * hrt_render_views, which stays a batch of pinhole cameras. */
enum { HRT_LENS_PERSPECTIVE = 0, HRT_LENS_ORTHOGRAPHIC = 1, HRT_LENS_EQUIRECT = 2, HRT_LENS_FISHEYE = 3 };
#define HRT_LENS_DRAW 0x80000000u   /* draw index of the first of the two lens draws */
typedef struct hrt_lens {
    hrt_camera cam;         /* eye + basis; must be a camera hrt_render accepts. fovy/znear/zfar are read by PERSPECTIVE only, aspect by all but EQUIRECT */
    uint32_t projection;    /* HRT_LENS_* */
    float aperture_radius;  /* >= 0, finite; 0 = pinhole. Must be 0 unless PERSPECTIVE */
    float focus_distance;   /* > 0 and finite when aperture_radius > 0: depth ALONG FORWARD of the plane in focus; ignored (any value) otherwise */
    float extent;           /* ORTHOGRAPHIC: height of the view volume in world units, > 0, finite. FISHEYE: full field of view in degrees, in (0, 360]. Otherwise must be 0 */
} hrt_lens;
HRT_API int hrt_lens_rays(const hrt_lens *lens, uint32_t w, uint32_t h, uint32_t sample, uint64_t seed, float *d_rays, void *stream);
HRT_API int hrt_render_lens_device(hrt_scene *scene, const hrt_lens *lens, uint32_t w, uint32_t h, uint32_t first_sample, uint32_t n_samples,
                                   uint64_t seed, uint32_t flags, float *d_frame, void *stream);
HRT_API int hrt_render_lens(hrt_scene *scene, const hrt_lens *lens, uint32_t w, uint32_t h, uint32_t spp, uint64_t seed, uint32_t flags,
                            float *out_rgb, hrt_stats *stats /* may be NULL */);
HRT_API int hrt_render_lens_features(hrt_scene *scene, const hrt_lens *lens, uint32_t w, uint32_t h, uint32_t first_sample, uint32_t n_samples,
                                     uint64_t seed, float *d_features, void *stream);

/* ---- Batched lens views: many lens cameras of one scene, every one a w x h frame, in ONE launch of the fused lens kernel.
 * The N views make one dense index space of n_views * w * h items; item i is pixel i % (w*h) of view i / (w*h), one lane per item
 * in the grid-stride loop of hrt_render_lens_device, so small frames (light-probe grids, skybox faces, light fields), which do not
 * fill the device one at a time, do so together.  A sample is keyed (seed of its view, pixel y*w + x inside its view, sample) --
 * neither by the item nor by a launch-wide seed -- and every view may differ in everything: projection, aperture, camera, seed.
 * CONTRACT: frame v is bit-identical to hrt_render_lens_device(scene, &views[v].lens, w, h, first_sample, n_samples, views[v].seed,
 * flags), for every scene, every mix of projections in one batch, every n_views and every permitted flag set.  By the lens
 * contracts it therefore equals hrt_lens_rays + hrt_trace_radiance per sample, and for pinhole views frame v of hrt_render_views.
 * hrt_render_lens_views_device: d_frames (device) receives n_views * h * w * 3 floats, view-major, each view row-major as
 * hrt_render_lens_device's: the means over samples [first_sample, first_sample + n_samples), or with HRT_RADIANCE_ACCUMULATE the
 * running sums, exactly as there.  Asynchronous on `stream`.  FLAGS: those of hrt_render_lens_device, refused by the same names and
 * texts; HRT_FLAG_GAMMA is applied in place over all frames and refused together with HRT_RADIANCE_ACCUMULATE.
 * hrt_render_lens_views: the same into a HOST buffer, blocking, samples [0, spp); stats as hrt_render_lens (samples = n_views * w *
 * h * spp; n_views == 0 zeroes them).  HRT_RADIANCE_ACCUMULATE is refused (the sums live on the device).
 * hrt_render_lens_views_features: block v of d_features (n_views * h * w * HRT_FEATURE_FLOATS floats, view-major) is bit-identical
 * to hrt_render_lens_features of views[v].lens with seed views[v].seed; n_samples == 0 is the pixel centres, as there.
 * CONCURRENCY: the per-view table (n_views lens blocks do not fit a kernel argument) is scratch of the scene: a grow-only device
 * buffer and a pinned staging copy, so `views` may be freed when a call returns.  A call waits on the host until the previous
 * call's upload has read the staging copy (not for its kernel), and batched lens launches of one scene on different streams are
 * ordered against each other, because they share the table.  Nothing of the trace launches' state (work-queue head, path pool,
 * camera blocks) is touched: a batch may overlap a render of the same scene on another stream, as single lens frames do.
 * LIMIT: n_views * w * h <= 2^31 - 1, the pixel limit of one lens frame (2^31 / 16 for the features, as hrt_render_lens_features).
 * Checked in this order before the scene and the library state, HRT_ERR_INVALID with hrt_last_error() naming the entry point and
 * the culprit: flags (the two frame forms); (n_views == 0 returns HRT_OK here and launches nothing;) views NULL; every lens as
 * hrt_lens_rays checks it, the message prefixed "views[<index>].lens"; the frame; n_samples == 0 (the two frame forms);
 * first_sample + n_samples > 2^32 (the features: > 2^32 - 1, as hrt_render_lens_features); the output pointer NULL or not 4-byte
 * aligned; the limit above; then a NULL scene. */
typedef struct hrt_lens_view {
    hrt_lens lens;
    uint64_t seed;
} hrt_lens_view;
HRT_API int hrt_render_lens_views_device(hrt_scene *scene, const hrt_lens_view *views, uint32_t n_views, uint32_t w, uint32_t h,
                                         uint32_t first_sample, uint32_t n_samples, uint32_t flags, float *d_frames, void *stream);
HRT_API int hrt_render_lens_views(hrt_scene *scene, const hrt_lens_view *views, uint32_t n_views, uint32_t w, uint32_t h,
                                  uint32_t spp, uint32_t flags, float *out_rgb, hrt_stats *stats /* may be NULL */);
HRT_API int hrt_render_lens_views_features(hrt_scene *scene, const hrt_lens_view *views, uint32_t n_views, uint32_t w, uint32_t h,
                                           uint32_t first_sample, uint32_t n_samples, float *d_features, void *stream);

/* ---- Adaptive lens frames: the per-tile sample counts of hrt_render_adaptive under any lens.
 * The rounds, the estimate and the counts are EXACTLY the rule stated at hrt_render_adaptive above, with the sums of
 * hrt_render_lens in place of hrt_render's: round 0 adds samples [0, min_spp/2) to every HRT_TILE x HRT_TILE tile, round 1 adds
 * [min_spp/2, min_spp) and judges every tile, every later round adds min(n, max_spp - n) samples to the tiles still active and judges
 * them, until none is active.  Every round is one launch of the fused lens kernel over the list of active tiles (one lane per
 * pixel of a listed tile, the lens a kernel argument), adding its samples in sample order onto the stored sums.  A DEGENERATE sample
 * (see THE RULE above) adds nothing and counts in the divisor; a tile whose samples are all degenerate -- a tile of a fisheye frame
 * wholly outside the image circle -- has tile_err 0, stops at min_spp and is all zeros.
 * CONTRACT A: every tile of the result is bit-identical to the same tile of hrt_render_lens(lens, w, h, count of that tile, seed,
 * flags), for every projection and every permitted flag set, HRT_FLAG_GAMMA included.
 * CONTRACT B: with HRT_LENS_PERSPECTIVE and aperture_radius == 0, frame and counts equal those of hrt_render_adaptive(&lens->cam, ...)
 * with the same parameters, seed and gamma flag, under every kernel form of that call.
 * hrt_render_lens_adaptive_device: d_frame (device, h*w*3 floats, ROW-MAJOR) receives the means (gamma-corrected with
 * HRT_FLAG_GAMMA), d_tile_spp (device, may be NULL) tiles_y * tiles_x uint32 counts, row-major.  Runs on `stream` (a hipStream_t,
 * NULL = the default stream) and synchronises it once per round from round 1 on, as hrt_render_adaptive_tiles does: one 4-byte
 * read-back (how many tiles are still active) sizes the next launch.  Every lens launch is checked for a HIP error when it is made;
 * a fault while a round runs ends the call with HRT_ERR_DEVICE at that round's synchronisation.
 * hrt_render_lens_adaptive: the same into HOST buffers out_rgb[h*w*3] and out_tile_spp (may be NULL), blocking.  stats (may be NULL):
 * kernel_ms = the lens kernels' time summed over all rounds (HIP events), samples = sum over in-image pixels of their tile's count
 * (degenerate samples count), as hrt_render_adaptive.
 * FLAGS: HRT_FLAG_EXACT_ONLY, HRT_FLAG_MESH_BRUTE (with EXACT_ONLY), HRT_FLAG_NO_LDS_TREE, HRT_FLAG_GAMMA.  HRT_RADIANCE_ACCUMULATE
 * (the rounds keep the running sums themselves) and every other bit are refused by name, with hrt_render_lens_device's texts.
 * Checked in this order before the scene and the library state, HRT_ERR_INVALID with hrt_last_error() naming the entry point and
 * the culprit: flags; params, as hrt_render_adaptive checks them; the lens, as hrt_lens_rays checks it; the frame; LIMIT:
 * hrt_tiles_total(w, h) * 64 <= 2^31 - 1 (one launch indexes 64 items per tile); d_frame / out_rgb NULL or not 4-byte aligned,
 * d_tile_spp / out_tile_spp not 4-byte aligned; then a NULL scene.
 * CONCURRENCY: the tile-major sums of the frame are a grow-only buffer of the scene's own; the tile lists and keep words are the
 * round scratch hrt_render_adaptive uses.  Nothing of the trace launches' state (work-queue head, path pool, camera blocks) is
 * touched: the call may overlap a plain render or a query of the same scene on another stream.  It may NOT overlap another
 * adaptive call of the same scene, lens or pinhole, because they share the round scratch.
 * OUT OF SCOPE: batched views (hrt_render_lens_views stays uniform), rank / world partitions (one device renders the whole
 * frame), the streaming kernel, and denoising of adaptive frames. */
HRT_API int hrt_render_lens_adaptive_device(hrt_scene *scene, const hrt_lens *lens, uint32_t w, uint32_t h, const hrt_adaptive *params,
                                            uint64_t seed, uint32_t flags, float *d_frame, uint32_t *d_tile_spp /* may be NULL */,
                                            void *stream);
HRT_API int hrt_render_lens_adaptive(hrt_scene *scene, const hrt_lens *lens, uint32_t w, uint32_t h, const hrt_adaptive *params,
                                     uint64_t seed, uint32_t flags, float *out_rgb, uint32_t *out_tile_spp /* may be NULL */,
                                     hrt_stats *stats /* may be NULL */);

/* ---- Baking: the radiance arriving at caller-supplied surface points (lightmaps, per-vertex irradiance) in one launch.
 * POINTS: n records of HRT_RAY_FLOATS floats (32 bytes, the array 16-byte aligned), device memory: the layout of a ray record with
 * the normal in place of the direction and the bias in place of tmax, {P.x, P.y, P.z, time, N.x, N.y, N.z, bias}.  Point i has the
 * key k = d_keys ? d_keys[i] : i.
 * THE RULE (the ray of sample s of point i; tests/bake_ref.py states it again in NumPy).  All arithmetic is fp32 without fused
 * multiply-add, in the order written; sqrtf, sinf, cosf and copysignf are the device's; normalize is the trace path's own (divide
 * by the length):
 *   Nn  = normalize(N)
 *   b0, b1 = draws 0 and 1 of stream (seed, k, s)   -- the slots the camera uses for u, v; a radiance path starts at draw 3
 *   r   = sqrtf(b0), phi = 6.2831855f * b1
 *   x   = r * cosf(phi), y = r * sinf(phi), z = sqrtf(1.f - b0)                       -- cosine-weighted about +z
 *   sg  = copysignf(1.f, Nn.z), a = -1.f / (sg + Nn.z), b = (Nn.x * Nn.y) * a          -- a branch-free frame without a pole
 *   T   = (1.f + (sg * (Nn.x * Nn.x)) * a, sg * b, (-sg) * Nn.x)
 *   B   = (b, sg + (Nn.y * Nn.y) * a, -Nn.y)
 *   d   = normalize((x * T + y * B) + z * Nn)
 *   O   = P + bias * Nn
 *   ray = {O, time, d, +inf}
 * `time` places the scene's moving objects; the point stays where it is.
 * DEGENERATE: a point is degenerate when one of its eight floats is not finite, bias < 0, N == 0, or Nn has a component that is not
 * finite or is 0 (a normal whose squared length underflows).  A sample is degenerate when its point is, or when a component of O or
 * d is not finite, or d == 0.  hrt_bake_rays writes a degenerate sample as {P, time, 0, 0, 0, +inf}: d == 0 is the query layer's own
 * rule for "not traced", the convention of hrt_lens_rays.  In a bake it adds nothing and still counts in the divisor: a degenerate
 * point gives 0 in mean mode and leaves its sums as they are under HRT_RADIANCE_ACCUMULATE, exactly as a degenerate ray does in
 * hrt_trace_radiance.
 * UNITS: the output is what hrt_trace_radiance gives, the mean over samples of radiance / 6.  The directions have the density
 * cos(theta) / pi about Nn, so the irradiance at the point is pi times the mean radiance; the calls apply NO factor.
 * hrt_bake_rays: the ray records of one sample (n records, device, 16-byte aligned) -- the sibling of hrt_camera_rays and
 * hrt_lens_rays.  No scene: it runs on the calling thread's current device, asynchronously on `stream`.
 * hrt_bake_device: the fused bake, 3 floats per point at d_out[3i .. 3i+2], with no ray buffer: the mean over samples
 * [first_sample, first_sample + n_samples), or with HRT_RADIANCE_ACCUMULATE the running sums, exactly as hrt_trace_radiance's
 * output.  Asynchronous on `stream`; touches none of the scene's per-launch state, so it may overlap a render of the same scene.
 * CONTRACT A: bit-identical to composing, for s in order, hrt_bake_rays(s) and hrt_trace_radiance(first_sample = s, n_samples = 1,
 * the same d_keys), summed in fp32 and divided by (float)n_samples -- for every scene and flag set.
 * Flags: HRT_FLAG_EXACT_ONLY, HRT_FLAG_MESH_BRUTE (with EXACT_ONLY), HRT_FLAG_NO_LDS_TREE, HRT_RADIANCE_ACCUMULATE.  Every other
 * bit is refused by name; that includes HRT_RAYS_NORMALIZE (the normal is always normalised), HRT_FLAG_GAMMA and the kernel-form
 * flags.
 * hrt_bake: the same from and into HOST buffers (`points`, `keys`, `out`; 4-byte aligned), blocking, samples [0, spp); stats as
 * hrt_render_lens (kernel_ms from events, samples = n * spp; n == 0 zeroes them).  HRT_RADIANCE_ACCUMULATE is refused (the sums
 * live on the device).
 * Checked in this order before the scene and the library state, HRT_ERR_INVALID with hrt_last_error() naming the entry point and
 * the culprit: flags; (n == 0 returns HRT_OK here and launches nothing;) d_points NULL or not 16-byte aligned; d_keys not 4-byte
 * aligned; n > 2^31 - 1; n_samples == 0; first_sample + n_samples > 2^32; the output NULL or misaligned (d_rays 16 bytes, d_out
 * 4); then a NULL scene.
 * POINT GENERATORS (host only: no device, no hrt_init; fp32 in the order written, restated in tests/bake_ref.py):
 * hrt_bake_quad_points writes tw * th records, row-major, texel (i, j) at index j*tw + i:
 *   P = (v0 + ((i + .5f)/tw) * (v1 - v0)) + ((j + .5f)/th) * (v3 - v0),  N = side * normalize(cross(v1 - v0, v3 - v0))
 * with side +1 or -1; +1 is the side the trace path lights (Square::intersect culls d.n > 0 for non-glass quads).
 * hrt_bake_mesh_points writes one record per vertex (positions: 3 floats per vertex, indices: 3 per triangle): N is the sum, over
 * the triangles that use the vertex in ascending triangle order, of cross(p1 - p0, p2 - p0), left unnormalised (the bake
 * normalises it); a vertex that no triangle uses gets N = 0, a degenerate point.  An index >= n_vertices is refused before
 * anything is written.
 * Both refuse (HRT_ERR_INVALID, by name) NULL pointers, tw or th zero, tw*th > 2^31 - 1, side other than +1 / -1, and a time or
 * bias that is not finite.
 * OUT OF SCOPE (DESIGN.md section 5 "Baking"): jitter inside a texel, points that follow a moving quad, sphere and mesh-texel
 * parametrisations, denoising of lightmaps, the streaming kernel, multi-GPU.  Spherical-harmonic probes are "Light probes" below. */
HRT_API int hrt_bake_rays(const float *d_points, const uint32_t *d_keys, uint32_t n, uint32_t sample, uint64_t seed, float *d_rays, void *stream);
HRT_API int hrt_bake_device(hrt_scene *scene, const float *d_points, const uint32_t *d_keys, uint32_t n, uint32_t first_sample,
                            uint32_t n_samples, uint64_t seed, uint32_t flags, float *d_out, void *stream);
HRT_API int hrt_bake(hrt_scene *scene, const float *points, const uint32_t *keys, uint32_t n, uint32_t spp, uint64_t seed, uint32_t flags,
                     float *out, hrt_stats *stats /* may be NULL */);
HRT_API int hrt_bake_quad_points(const hrt_quad *quad, uint32_t tw, uint32_t th, int32_t side, float time, float bias, float *out_points);
HRT_API int hrt_bake_mesh_points(const float *positions, uint32_t n_vertices, const uint32_t *indices, uint32_t n_triangles, float time,
                                 float bias, float *out_points);

/* ---- Light probes: the radiance arriving at caller-supplied points in space from EVERY direction, projected onto the 9 real
 * spherical-harmonic (SH) basis functions of bands 0..2, per colour channel, in one launch.
 * PROBES: n records of HRT_PROBE_FLOATS floats (16 bytes, the array 16-byte aligned), device memory: {P.x, P.y, P.z, time}.  Probe i
 * has the key k = d_keys ? d_keys[i] : i.  A probe is DEGENERATE when one of its four floats is not finite.
 * THE RULE (tests/probe_ref.py states it again in NumPy).  All arithmetic is fp32 without fused multiply-add, in the order written;
 * sqrtf, sinf and cosf are the device's; normalize is the trace path's own (divide by the length).
 * Direction of sample s of probe i, uniform on the sphere:
 *   b0, b1 = draws 0 and 1 of stream (seed, k, s)   -- the slots a bake uses; a radiance path starts at draw 3
 *   z = 1.f - 2.f * b0, r = sqrtf(fmaxf(0.f, 1.f - z * z)), phi = 6.2831855f * b1
 *   d = normalize((r * cosf(phi), r * sinf(phi), z))
 *   ray = {P, time, d, +inf}
 * A sample is degenerate when its probe is, or when a component of d is not finite, or d == 0.  hrt_probe_rays writes it as
 * {P, time, 0, 0, 0, +inf}; it adds nothing and still counts in the divisor -- the convention of hrt_bake_rays.
 * Basis, with (x, y, z) = d:
 *   Y0 = 0.2820948f
 *   Y1 = 0.48860251f * y        Y2 = 0.48860251f * z        Y3 = 0.48860251f * x
 *   Y4 = 1.0925485f * (x * y)   Y5 = 1.0925485f * (y * z)
 *   Y6 = 0.31539157f * (3.f * (z * z) - 1.f)
 *   Y7 = 1.0925485f * (x * z)   Y8 = 0.54627422f * (x * x - y * y)
 * The sum.  Its order is fixed and does not depend on how the device schedules it.  v(s) is the three floats
 * hrt_trace_radiance(first_sample = s, n_samples = 1) returns for the ray above (that path's radiance / 6), j = s - first_sample:
 *   sample j belongs to block j / HRT_PROBE_BLOCK and to lane j % 64 of that block;
 *   lane partial: a[k][c] = 0.f, then for the lane's samples in ascending j: a[k][c] = a[k][c] + Y_k * v_c (one multiply and one
 *     add per term; a degenerate sample adds nothing; a lane with no samples holds 0.f);
 *   block value: halving over the 64 lane partials: for m = 32, 16, 8, 4, 2, 1: a_l = a_l + a_{l+m} for l < m; the value is a_0;
 *   total: t = 0.f, then t = t + block_b for b ascending;
 *   output: 27 floats per probe, d_out[27 i + 3 k + c]: t / (float)n_samples, or with HRT_RADIANCE_ACCUMULATE d_out (on entry) + t.
 * UNITS: the output is the mean over uniform directions of Y_k(d) times what hrt_trace_radiance gives (radiance / 6); the calls
 * apply NO factor, as the bakes.  The SH coefficients of the incoming radiance are 4 pi * 6 * the mean.  (The irradiance evaluator
 * is "Probe volumes" below: it convolves with the clamped cosine by scaling band 0 by pi, band 1 by 2 pi / 3 and band 2 by pi / 4
 * -- Ramamoorthi and Hanrahan 2001 -- and evaluates the basis at the normal, between the eight probes round a point.)
 * hrt_probe_rays: the ray records of one sample (n records of HRT_RAY_FLOATS floats, device, 16-byte aligned) -- the sibling of
 * hrt_bake_rays.  No scene: it runs on the calling thread's current device, asynchronously on `stream`.
 * hrt_probes_device: the fused form, with no ray buffer, asynchronous on `stream`.  One wave of the device works on one (probe,
 * block) pair, its lane the rule's lane; a second small launch on the same stream adds the block values.
 * CONTRACT A: bit-identical to the sum above over the per-sample outputs of hrt_probe_rays(s) and hrt_trace_radiance(first_sample = s,
 * n_samples = 1, the same d_keys) -- for every scene and flag set.
 * Flags: a bake's -- HRT_FLAG_EXACT_ONLY, HRT_FLAG_MESH_BRUTE (with EXACT_ONLY), HRT_FLAG_NO_LDS_TREE, HRT_RADIANCE_ACCUMULATE.  Every
 * other bit is refused by name; that includes HRT_RAYS_NORMALIZE (a probe has no direction to normalise), HRT_FLAG_GAMMA and the
 * kernel-form flags.
 * hrt_probes: the same from and into HOST buffers (`probes`, `keys`, `out`; 4-byte aligned), blocking, samples [0, spp); stats as
 * hrt_bake (samples = n * spp; n == 0 zeroes them).  HRT_RADIANCE_ACCUMULATE is refused (the sums live on the device).
 * LIMIT: n * ceil(n_samples / HRT_PROBE_BLOCK) <= HRT_PROBE_MAX_BLOCKS: the block values stay below 453 MB and a work item times
 * 64 fits 32 bits.
 * Checked in this order before the scene and the library state, HRT_ERR_INVALID with hrt_last_error() naming the entry point and
 * the culprit: flags; (n == 0 returns HRT_OK here and launches nothing;) d_probes NULL or not 16-byte aligned; d_keys not 4-byte
 * aligned; n > 2^31 - 1; n_samples == 0; first_sample + n_samples > 2^32; the limit above; the output NULL or misaligned (d_rays
 * 16 bytes, d_out 4); then a NULL scene.
 * CONCURRENCY: the block values are a grow-only scratch buffer of the scene's, allocated by its first probe call and freed with
 * the scene, so probe launches of ONE scene must not overlap each other.  Nothing of the trace launches' per-launch state is
 * touched: a probe launch may overlap a render or a query of the same scene on another stream.
 * hrt_probe_grid_points (host only: no device, no hrt_init; fp32 in the order written) writes nx * ny * nz records, probe (i, j, k)
 * at index (k*ny + j)*nx + i, per axis at lo + ((i + .5f)/nx) * (hi - lo); lo > hi on an axis runs it backwards.  It refuses
 * (HRT_ERR_INVALID, by name) NULL pointers, a zero count, nx*ny*nz > 2^31 - 1 and a lo, hi or time that is not finite.
 * OUT OF SCOPE (DESIGN.md section 5 "Light probes"): higher SH orders, stratified or low-discrepancy directions, probes that move,
 * the streaming kernel, multi-GPU (a caller splits the probes; the keys keep every probe's random numbers).  The irradiance
 * evaluator is "Probe volumes" below; depth moments per probe are "Probe visibility". */
#define HRT_PROBE_FLOATS 4
#define HRT_PROBE_COEFFS 9
#ifndef HRT_PROBE_BLOCK
#define HRT_PROBE_BLOCK 64u           /* samples per block of the sum; a multiple of 64 (-DHRT_PROBE_BLOCK: the A/B builds) */
#endif
#define HRT_PROBE_MAX_BLOCKS (1u << 22)
HRT_API int hrt_probe_rays(const float *d_probes, const uint32_t *d_keys, uint32_t n, uint32_t sample, uint64_t seed, float *d_rays, void *stream);
HRT_API int hrt_probes_device(hrt_scene *scene, const float *d_probes, const uint32_t *d_keys, uint32_t n, uint32_t first_sample,
                              uint32_t n_samples, uint64_t seed, uint32_t flags, float *d_out, void *stream);
HRT_API int hrt_probes(hrt_scene *scene, const float *probes, const uint32_t *keys, uint32_t n, uint32_t spp, uint64_t seed, uint32_t flags,
                       float *out, hrt_stats *stats /* may be NULL */);
HRT_API int hrt_probe_grid_points(const float *lo, const float *hi, uint32_t nx, uint32_t ny, uint32_t nz, float time, float *out_probes);

/* ---- Probe volumes: a regular grid of the SH9 probes above that lives on the device, evaluated at caller-supplied SURFACE POINTS
 * (lightmap texels, mesh vertices, the first hits of a frame) in one launch: each point is interpolated between the eight probes
 * round it and gives the irradiance -- or the radiance -- in the direction of its normal, in the units of hrt_bake.
 * GRID: that of hrt_probe_grid_points.  Probe (i, j, k) is at index (k*ny + j)*nx + i, per axis at lo + ((i + .5f)/n) * (hi - lo);
 * lo > hi on an axis runs it backwards.  hrt_probe_volume_create computes per axis, on the host in fp32, e = hi - lo and
 * s = (float)n / e (s is not used on an axis with n == 1) and refuses (HRT_ERR_INVALID, by name) NULL pointers, a zero count,
 * nx*ny*nz > HRT_PROBE_VOLUME_MAX, a lo or hi that is not finite, e == 0 on an axis with n > 1, and an s that is not finite.
 * COEFFICIENTS: nx*ny*nz * 27 floats, the layout hrt_probes* writes (d_out[27 i + 3 k + c]), taken unscaled.  An update repacks
 * them (hrt_probe_pack_kernel) into records of HRT_PROBE_RECORD_FLOATS floats -- the 27 followed by 5 zeros, 128 bytes on a
 * 128-byte boundary -- so that each corner of a look-up is one aligned line; the caller's buffer is free when the launch has run
 * (hrt_probe_volume_update_device, asynchronous on `stream`) or on return (hrt_probe_volume_update, host buffer, blocking).
 * POINTS: the bake's records, n * HRT_RAY_FLOATS floats {P.x, P.y, P.z, time, N.x, N.y, N.z, bias}, 16-byte aligned on the device:
 * the output of hrt_bake_quad_points and hrt_bake_mesh_points goes in as it is.  `time` and `bias` are not read.  A point is
 * DEGENERATE when a float of P or N is not finite, when N == 0, or when Nn = normalize(N) has a component that is not finite (a
 * normal whose squared length underflows); it gives three zeros.
 * THE RULE (tests/probe_volume_ref.py states it again in NumPy).  All arithmetic is fp32 without fused multiply-add, in the order
 * written; it uses only + - * /, sqrtf, floorf, fminf and fmaxf (of which a NaN operand is dropped); normalize is the trace path's
 * own (divide by the length):
 *   1. per axis with n > 1: g = fminf(fmaxf((P - lo) * s - .5f, 0.f), (float)(n - 1)), i0 = (uint32_t)floorf(g), f = g - (float)i0,
 *      i1 = min(i0 + 1, n - 1); with n == 1: i0 = i1 = 0, f = 0.f.  Points outside the box clamp to the outermost probes.
 *   2. corner m = 0..7: bit 0 of m chooses x, bit 1 y, bit 2 z; the per-axis weight is 1.f - f for the 0 side and f for the 1
 *      side; w_m = (wx * wy) * wz.
 *   3. with HRT_PROBE_EVAL_FACING (the back-face term of dynamic diffuse global illumination, Majercik et al. 2019): C_m the
 *      corner's centre by the grid formula, v = C_m - P, l = sqrtf((v.x*v.x + v.y*v.y) + v.z*v.z),
 *      c = l > 0.f ? ((v.x*Nn.x + v.y*Nn.y) + v.z*Nn.z) / l : 0.f, t = (c + 1.f) * .5f, w_m = w_m * (t * t + .2f); then
 *      W = ((((((w_0 + w_1) + w_2) + w_3) + w_4) + w_5) + w_6) + w_7 and w_m = w_m / W.  W > 0: every factor is at least .2 and
 *      some trilinear weight is positive.  (A P so far away that l overflows gives NaN.)
 *   4. for each of the 27 slots j = 3k + ch: a_j = 0.f, then for m ascending a_j = a_j + w_m * p_m[j], p_m the corner's
 *      coefficients.
 *   5. Y_k: the basis of "Light probes", the same constants and expressions, at (x, y, z) = Nn.
 *   6. out[ch] = 0.f, then for k ascending out[ch] = out[ch] + (F_k * a_{3k+ch}) * Y_k, with F per band:
 *        irradiance (default):            12.566371f (4 pi) for k = 0, 8.3775804f (8 pi / 3) for k = 1..3, 3.1415927f (pi) for k = 4..8;
 *        with HRT_PROBE_EVAL_RADIANCE:    12.566371f for every k.
 * The result does not depend on how the device maps points to lanes.
 * UNITS: the default output is the irradiance divided by pi in hrt_trace_radiance's units (radiance / 6) -- exactly what hrt_bake
 * returns for the same record; a constant environment of value L gives L.  Derivation: a probe holds the means
 * c_k = (1 / 4 pi) x the integral of Y_k L over the sphere, so the SH coefficients of L are L_k = 4 pi c_k; convolving with the
 * clamped cosine scales band 0 by pi, band 1 by 2 pi / 3 and band 2 by pi / 4 (Ramamoorthi and Hanrahan 2001); dividing by pi
 * gives F = 4 pi, 8 pi / 3, pi.  With HRT_PROBE_EVAL_RADIANCE the output is the SH reconstruction of the radiance arriving from
 * direction Nn, in the same units.
 * hrt_probe_eval_device: 3 floats per point at d_out[3i .. 3i+2], asynchronous on `stream`.  hrt_probe_eval: the same from and into
 * HOST buffers (4-byte aligned), blocking; stats as hrt_bake (kernel_ms from events, samples = n; n == 0 zeroes them).
 * hrt_probe_volume_weights (host only: no device, no hrt_init): steps 1-3 for ONE point record -- the eight probe indices and the
 * final weights, by the code the kernel runs (csrc/hrt_probe_volume_cell.h); both zeroed, and HRT_OK, for a degenerate point.  It
 * refuses what create refuses, unknown flags, and NULL point, index or weight.
 * Checked in this order, HRT_ERR_INVALID with hrt_last_error() naming the entry point and the culprit: flags (every bit beyond the
 * two refused by name); (n == 0 returns HRT_OK here and launches nothing;) the volume NULL; a volume never updated ("has no
 * coefficients yet"); the points NULL or misaligned (16 bytes on the device, 4 on the host); n > 2^31 - 1; the output NULL or not
 * 4-byte aligned.  The updates: the volume NULL, the coefficients NULL or not 4-byte aligned.  The library state comes after these,
 * as for hrt_denoise: HRT_ERR_STATE before hrt_init -- which create needs too, since it allocates.
 * CONCURRENCY AND LIFETIME: an evaluation only reads the volume, so evaluations may overlap each other and any launch of any scene.
 * An update must not overlap an evaluation of the same volume; on one stream they are ordered.  The volume needs no scene: it
 * belongs to the device that was current at create (one hrt_init has prepared), every call on it makes that device current, and
 * its buffer is counted by hrt_debug_live_resources until hrt_probe_volume_destroy, which waits for the launches that read it.
 * OUT OF SCOPE (DESIGN.md section 5 "Probe volumes"): probes that move, higher SH orders, multi-GPU.  Visibility (Chebyshev leak
 * tests on depth moments per probe) is "Probe visibility" below; the probe-lit frame and a volume that relights itself are "Lit
 * rays". */
typedef struct hrt_probe_volume hrt_probe_volume;
#define HRT_PROBE_VOLUME_MAX (1u << 24)   /* probes: the packed copy stays at or below 2 GiB */
#define HRT_PROBE_RECORD_FLOATS 32        /* packed record: 27 coefficients + 5 zeros, 128 bytes, 128-byte aligned */
#define HRT_PROBE_EVAL_RADIANCE 1u        /* SH radiance in direction N instead of cosine-convolved */
#define HRT_PROBE_EVAL_FACING 2u          /* weight probes by how far they face the surface */
HRT_API int hrt_probe_volume_create(const float *lo, const float *hi, uint32_t nx, uint32_t ny, uint32_t nz, hrt_probe_volume **out);
HRT_API int hrt_probe_volume_update_device(hrt_probe_volume *volume, const float *d_coeffs, void *stream);
HRT_API int hrt_probe_volume_update(hrt_probe_volume *volume, const float *coeffs);
HRT_API void hrt_probe_volume_destroy(hrt_probe_volume *volume);
HRT_API int hrt_probe_eval_device(const hrt_probe_volume *volume, const float *d_points, uint32_t n, uint32_t flags, float *d_out, void *stream);
HRT_API int hrt_probe_eval(const hrt_probe_volume *volume, const float *points, uint32_t n, uint32_t flags, float *out,
                           hrt_stats *stats /* may be NULL */);
HRT_API int hrt_probe_volume_weights(const float *lo, const float *hi, uint32_t nx, uint32_t ny, uint32_t nz, const float *point, uint32_t flags,
                                     uint32_t index[8], float weight[8]);

/* ---- Probe visibility: depth moments per probe and a look-up that does not leak through walls.  A plain look-up interpolates
 * between the eight probes round a point whether or not they can see it; here every probe also gets a small map of the mean
 * distance and the mean squared distance to the scene per direction, and the look-up turns the two moments into a Chebyshev
 * visibility weight per corner (the variance shadow-map test of dynamic diffuse global illumination, Majercik et al. 2019).
 * THE RULE (tests/probe_depth_ref.py states it again in NumPy).  All arithmetic is fp32 without fused multiply-add, in the order
 * written; it uses only + - * /, sqrtf, floorf, fabsf, fminf and fmaxf; sg(v) = v >= 0.f ? 1.f : -1.f.
 * DEPTH MAP: HRT_PROBE_DEPTH_RES x HRT_PROBE_DEPTH_RES = HRT_PROBE_DEPTH_TEXELS texels per probe in octahedral parametrisation,
 * texel e = 8 j + i.
 *   Centre direction c_e: px = ((float)i + .5f) * .25f - 1.f, py likewise from j; z = (1.f - fabsf(px)) - fabsf(py); if z < 0.f:
 *     (px, py) = ((1.f - fabsf(py)) * sg(px), (1.f - fabsf(px)) * sg(py)), computed from the old pair; c_e = normalize((px, py, z)),
 *     the trace path's own normalize (divide by the length).
 *   Texel of a vector v != 0, which need not be unit: s = (fabsf(v.x) + fabsf(v.y)) + fabsf(v.z); px = v.x / s, py = v.y / s; if
 *     v.z < 0.f the same fold; i = (uint32_t)fminf(fmaxf(floorf((px * .5f + .5f) * 8.f), 0.f), 7.f), j likewise from py.
 *   Both are csrc/hrt_probe_depth_oct.h, shared by the kernels, the host and a sanitized stand-alone program; hrt_probe_depth_texel
 *   and hrt_probe_depth_direction (host only: no device, no hrt_init) expose them and refuse NULL pointers and a texel >=
 *   HRT_PROBE_DEPTH_TEXELS.
 * DEPTH SAMPLE: sample s of probe i uses the direction d of "Light probes" -- probe_dir(seed, key, s), unchanged, so the depth map
 * sees the directions the SH coefficients saw.  r(s) = fminf(t, r_max), t being what hrt_trace_rays(HRT_QUERY_CLOSEST) returns
 * for the record hrt_probe_rays writes for that sample under the same trace flags (its per-ray margin and far-origin rule
 * included); a miss gives r_max; a degenerate sample adds nothing.  r_max is the caller's, finite and > 0.
 * THE SUM.  Its order is fixed.  With j = s - first_sample, sample j belongs to block j / 64.  Block value of texel e: W = A = B =
 * 0.f, then for the block's non-degenerate samples in ascending j:
 *     w = fmaxf(0.f, (c_e.x*d.x + c_e.y*d.y) + c_e.z*d.z); w = w*w, five times (the 32nd power);
 *     W = W + w; A = A + w * r; B = B + w * (r * r).
 *   total: t = 0.f, then t = t + block_b for b ascending.
 *   output: HRT_PROBE_DEPTH_FLOATS = 192 floats per probe, d_out[192 i + 3 e + {0, 1, 2}] = {W, A, B}: sums, not means; with
 *   HRT_RADIANCE_ACCUMULATE d_out (on entry) + t.
 * hrt_probe_depth_device: asynchronous on `stream`; one wave of the device works on one (probe, block) pair, a lane is one sample
 * and then one texel; a second small launch on the same stream adds the block values.  hrt_probe_depth: the same from and into
 * HOST buffers (4-byte aligned), blocking, samples [0, spp); stats as hrt_probes; HRT_RADIANCE_ACCUMULATE is refused there.
 * CONTRACT A: bit-identical to the sum above over the per-sample outputs of hrt_probe_rays(s) and hrt_trace_rays(HRT_QUERY_CLOSEST)
 * -- for every scene and flag set.
 * Flags of a depth launch: HRT_FLAG_EXACT_ONLY, HRT_FLAG_MESH_BRUTE (with EXACT_ONLY), HRT_FLAG_NO_LDS_TREE,
 * HRT_RADIANCE_ACCUMULATE; every other bit is refused by name.
 * LIMIT: n * ceil(n_samples / 64) <= HRT_PROBE_DEPTH_MAX_BLOCKS: the block values stay at or below 805 MB.
 * Checked in this order before the scene and the library state, HRT_ERR_INVALID with hrt_last_error() naming the entry point and
 * the culprit: flags; (n == 0 returns HRT_OK here and launches nothing;) the probe records NULL or misaligned (16 bytes on the
 * device, 4 on the host), the keys not 4-byte aligned; n > 2^31 - 1, n_samples == 0, first_sample + n_samples > 2^32, the limit;
 * r_max not finite or not positive; the output NULL or not 4-byte aligned; then a NULL scene.
 * CONCURRENCY: the block values are a grow-only scratch buffer of the scene's own, allocated by its first depth call and freed
 * with the scene, so depth launches of ONE scene must not overlap each other; they may overlap anything else.
 * MOMENTS: hrt_probe_volume_update_depth* takes the sums of the volume's nx*ny*nz probes (192 floats each) and keeps one pair per
 * texel (hrt_probe_depth_pack_kernel): W > 0.f ? {A / W, B / W} : {+inf, 0.f} -- a texel nobody looked through hides nothing.
 * 512 bytes per probe in a second buffer of the volume's, allocated by the first depth update, counted by
 * hrt_debug_live_resources and freed with the volume.  Depth needs nx*ny*nz <= HRT_PROBE_DEPTH_VOLUME_MAX.  The updates refuse, in
 * this order: the volume NULL, the sums NULL or not 4-byte aligned, a volume of more probes than that; then the library state.
 * LOOK-UP WITH VISIBILITY (hrt_probe_eval_visible*): steps 1, 2, 4, 5 and 6 of "Probe volumes" word for word; step 3 becomes
 *   (a) with HRT_PROBE_EVAL_FACING the facing factor exactly as there, without its normalisation;
 *   (b) always the visibility factor, for corner m with centre C_m: Pb = P + b * Nn, b the record's `bias` float (which the plain
 *       look-up ignores; a b that is not finite makes the point degenerate); v = Pb - C_m;
 *       l = sqrtf((v.x*v.x + v.y*v.y) + v.z*v.z); if l > 0.f: {m1, m2} is corner m's texel of v; vis = 1.f when l <= m1, otherwise
 *       var = fmaxf(m2 - m1*m1, 0.f), q = l - m1, c = var / (var + q*q), vis = fmaxf((c*c)*c, .001f); l == 0.f gives vis = 1.f;
 *       w_m = w_m * vis;
 *   (c) always W = ((((((w_0 + w_1) + w_2) + w_3) + w_4) + w_5) + w_6) + w_7 and w_m = w_m / W.  The floor of .001 keeps W > 0.
 * Flags: HRT_PROBE_EVAL_RADIANCE and HRT_PROBE_EVAL_FACING; every other bit is refused by name.  Checked in the order of
 * hrt_probe_eval: flags; (n == 0 returns HRT_OK;) the volume NULL; a volume without coefficients ("has no coefficients yet"); a
 * volume without depth ("has no depth moments yet"); the points; n; the output; then the library state.  An evaluation only reads
 * the volume; a depth update must not overlap an evaluation of the same volume.
 * OUT OF SCOPE (DESIGN.md section 5 "Probe visibility"): bilinear texel look-up, DDGI's weight crush, a view-dependent bias,
 * probes that move. */
#define HRT_PROBE_DEPTH_RES 8u
#define HRT_PROBE_DEPTH_TEXELS 64u               /* RES x RES */
#define HRT_PROBE_DEPTH_FLOATS 192u              /* per probe: {W, A, B} per texel */
#define HRT_PROBE_DEPTH_MAX_BLOCKS (1u << 20)
#define HRT_PROBE_DEPTH_VOLUME_MAX (1u << 22)    /* probes of a volume with depth: the moments stay at or below 2 GiB */
HRT_API int hrt_probe_depth_device(hrt_scene *scene, const float *d_probes, const uint32_t *d_keys, uint32_t n, uint32_t first_sample,
                                   uint32_t n_samples, uint64_t seed, float r_max, uint32_t flags, float *d_out, void *stream);
HRT_API int hrt_probe_depth(hrt_scene *scene, const float *probes, const uint32_t *keys, uint32_t n, uint32_t spp, uint64_t seed, float r_max,
                            uint32_t flags, float *out, hrt_stats *stats /* may be NULL */);
HRT_API int hrt_probe_volume_update_depth_device(hrt_probe_volume *volume, const float *d_sums, void *stream);
HRT_API int hrt_probe_volume_update_depth(hrt_probe_volume *volume, const float *sums);
HRT_API int hrt_probe_eval_visible_device(const hrt_probe_volume *volume, const float *d_points, uint32_t n, uint32_t flags, float *d_out,
                                          void *stream);
HRT_API int hrt_probe_eval_visible(const hrt_probe_volume *volume, const float *points, uint32_t n, uint32_t flags, float *out,
                                   hrt_stats *stats /* may be NULL */);
HRT_API int hrt_probe_depth_texel(const float v[3], uint32_t *texel);
HRT_API int hrt_probe_depth_direction(uint32_t texel, float out[3]);

/* ---- Lit rays: the radiance of a ray whose path ENDS in a probe volume at its first hit -- one closest hit, the hit shaded as the
 * integrator shades it, and everything beyond the hit taken from the volume as it stands.  It has two shapes: a ray query
 * (hrt_trace_lit: the probe-lit frame, noise-free at one sample but for the direct light), and a fused probe update
 * (hrt_probes_lit*), whose output goes back into the volume: each round of trace, look up, write back adds one bounce (the update of
 * dynamic diffuse global illumination, Majercik et al. 2019).
 * THE RULE (tests/probe_lit_ref.py states it again in NumPy).  All arithmetic is fp32 without fused multiply-add, in the order
 * written.  For a ray {o, time, d, tmax} (tmax is not read, as in hrt_trace_radiance), key k and sample s:
 *   1. RNG: stream (seed, k, s) with the draw index set to 3 -- the state of a path of hrt_trace_radiance at its first segment.  The
 *      filter margin and the far-origin rule are those of that first segment (DESIGN.md section 5 "Ray queries").  A ray is
 *      DEGENERATE exactly when hrt_trace_radiance calls it so (HRT_RAYS_NORMALIZE included); it adds nothing: 0 in mean mode, its
 *      sums left as they are under HRT_RADIANCE_ACCUMULATE.
 *   2. h = the closest hit of the ray, meshes included.
 *   3. a miss: rad = 0 + 1 * sky(d, 6), as the integrator writes it; value = rad / 6.f per channel -- the bits of a one-sample
 *      hrt_trace_radiance of a ray that misses.
 *   4. a hit: sf = the shaded surface; direct = the direct light at sf with the sample's stream (scenes with lights; 0 otherwise);
 *      rad = 0 + 1 * (direct + sf.emission); thr = 1 * sf.albedo -- the integrator's own expressions and device functions.
 *   5. the tail: for a diffuse surface G = the look-up of the point record {sf.p, time, sf.n, bias} -- sf.p = o + t * d, sf.n the
 *      shaded normal (NOT flipped towards the ray: the normal the integrator would scatter about) -- by THE RULE of "Probe volumes",
 *      steps 1-6 in irradiance form, or with HRT_LIT_VISIBLE by that of "Probe visibility"; HRT_PROBE_EVAL_FACING is passed through.
 *      A degenerate point record gives G = 0.  For mirror and glass G = 0: the chain is not followed.
 *      value = (rad / 6.f) + thr * G per channel.
 *   6. samples in ascending order: sum = 0.f (or d_out on entry, under HRT_RADIANCE_ACCUMULATE), sum = sum + value; the output is
 *      sum / (float)n_samples, or the running sum.
 * hrt_trace_lit: n ray records (device, HRT_RAY_FLOATS floats each, 16-byte aligned), 3 floats per ray at d_out[3i .. 3i+2]; ray i
 * has the key d_keys ? d_keys[i] : i.  One lane of the device per ray.  `flags` are hrt_trace_radiance's: HRT_FLAG_EXACT_ONLY,
 * HRT_FLAG_MESH_BRUTE (with EXACT_ONLY), HRT_FLAG_NO_LDS_TREE, HRT_RAYS_NORMALIZE, HRT_RADIANCE_ACCUMULATE.  `eval_flags`:
 * HRT_PROBE_EVAL_FACING and HRT_LIT_VISIBLE; HRT_PROBE_EVAL_RADIANCE is refused by name.  Asynchronous on `stream`; touches no
 * per-launch state of the scene.  Where no ray can continue past its first hit (a one-sided emitter under a dark sky) and the
 * volume holds zeros, the output is hrt_trace_radiance's bit for bit.
 * hrt_probes_lit_device: the same for the samples of probes -- records {P, time} as "Light probes", sample s of a probe the ray
 * {P, time, d(s), +inf} of hrt_probe_rays -- summed by the sum of "Light probes" with v(s) = 0.f + value(s): n x 27 coefficients in
 * the layout of hrt_probes*, the same blocks, lanes, halving and second launch.  One wave of the device works on one (probe, block)
 * pair; a sample is one segment, so the kernel has a body of its own without the integrator's stages.  `flags` are a probe launch's.
 * CONTRACT A: bit-identical to that sum over the per-sample outputs of hrt_probe_rays(s) and hrt_trace_lit(first_sample = s,
 * n_samples = 1, the same d_keys, eval_flags and bias) -- for every scene, volume and flag set.
 * hrt_probes_lit: the same from and into HOST buffers (4-byte aligned), blocking, samples [0, spp); stats as hrt_probes;
 * HRT_RADIANCE_ACCUMULATE is refused there.  LIMIT: that of hrt_probes*.
 * hrt_probe_volume_blend_device / hrt_probe_volume_blend: the hysteresis update on the packed records of a volume that has been
 * updated before: for each of the 27 coefficients p = (keep * p) + ((1.f - keep) * c); the five padding floats of a record stay 0.
 * keep = 0 gives hrt_probe_volume_update's bits for finite p.  They refuse, in this order: the volume NULL, the coefficients NULL or
 * not 4-byte aligned, a keep outside [0, 1) (NaN included), a volume never updated; then the library state.
 * Checked in this order, HRT_ERR_INVALID with hrt_last_error() naming the entry point and the culprit: flags; eval_flags
 * (HRT_PROBE_EVAL_RADIANCE by name, then unknown bits); the volume NULL; a volume never updated ("has no coefficients yet");
 * HRT_LIT_VISIBLE on a volume without depth ("has no depth moments yet"); a bias that is not finite; (n == 0 returns HRT_OK here and
 * launches nothing;) the rays or probe records NULL or misaligned, the keys not 4-byte aligned; for hrt_trace_lit the output NULL or
 * misaligned, then n > 2^31 - 1, n_samples == 0 and first_sample + n_samples > 2^32; for hrt_probes_lit* n, n_samples, first_sample,
 * the limit and the output in the order of hrt_probes*; then a NULL scene, a volume that lives on another device than the scene,
 * and the library state.
 * CONCURRENCY: a call only READS the volume, so lit launches may overlap look-ups of the same volume; an update or a blend of the
 * volume must be ordered after the lit launches that read it by the caller (on one stream they are).  The block values of
 * hrt_probes_lit* are a grow-only scratch buffer of the scene's own, allocated by its first such call and freed with the scene, so
 * lit probe launches of ONE scene must not overlap each other; they may overlap anything else.
 * OUT OF SCOPE (DESIGN.md section 5 "Lit rays and probe relighting"): a cooperative (eight lanes to a hit) look-up inside the kernels,
 * probes that move, multi-GPU.  Following mirror and glass to the first diffuse hit, and more than one segment before the tail, are
 * "Lit paths" below: these entry points keep their one segment and their bits. */
#define HRT_LIT_VISIBLE 4u                /* eval_flags of a lit launch: the look-up of "Probe visibility" */
HRT_API int hrt_trace_lit(hrt_scene *scene, const hrt_probe_volume *volume, const float *d_rays, const uint32_t *d_keys, uint32_t n,
                          uint32_t first_sample, uint32_t n_samples, uint64_t seed, uint32_t flags, uint32_t eval_flags, float bias,
                          float *d_out, void *stream);
HRT_API int hrt_probes_lit_device(hrt_scene *scene, const hrt_probe_volume *volume, const float *d_probes, const uint32_t *d_keys, uint32_t n,
                                  uint32_t first_sample, uint32_t n_samples, uint64_t seed, uint32_t flags, uint32_t eval_flags, float bias,
                                  float *d_out, void *stream);
HRT_API int hrt_probes_lit(hrt_scene *scene, const hrt_probe_volume *volume, const float *probes, const uint32_t *keys, uint32_t n, uint32_t spp,
                           uint64_t seed, uint32_t flags, uint32_t eval_flags, float bias, float *out, hrt_stats *stats /* may be NULL */);
HRT_API int hrt_probe_volume_blend_device(hrt_probe_volume *volume, const float *d_coeffs, float keep, void *stream);
HRT_API int hrt_probe_volume_blend(hrt_probe_volume *volume, const float *coeffs, float keep);

/* ---- Lit paths: a path of the integrator that ENDS in a probe volume at its K-th diffuse hit.  It is hrt_trace_radiance's path --
 * bounce loop, meshes, direct light, sky -- with one hook: at the K-th diffuse surface the path does not scatter but gathers from the
 * volume, as a lit ray does at its first hit.  Mirror and glass are followed (they cost a bounce and do not count towards K), so
 * K = 1 is "Lit rays" with specular chains followed, and K = 2 or 3 is final gathering: K - 1 real diffuse bounces, then the volume.
 * The same hook can write the path's end out instead of gathering there (hrt_path_tails): vertex, throughput and radiance so far.
 * THE RULE (tests/lit_paths_ref.py states it again in NumPy).  All arithmetic is fp32 without fused multiply-add, in the order
 * written.  For a ray {o, time, d, tmax} (tmax is not read), key k, sample s and tail_after = K in 1 .. HRT_MAXBOUNCES:
 *   1. the path starts as a path of hrt_trace_radiance starts: stream (seed, k, s) with the draw index set to 3, the filter margin
 *      and far-origin rule of a first segment, the same DEGENERATE rays (which add nothing); thr = 1, rad = 0, remaining = 6, and a
 *      counter diffuse = 0.
 *   2. per segment: h = the closest hit, meshes included.  A miss: rad = rad + thr * sky(d, remaining); the path ends with
 *      value = rad / 6.f per channel and NO TAIL.
 *   3. a hit: sf = the shaded surface; direct = the direct light at sf with the sample's stream (scenes with lights; 0 otherwise);
 *      rad = rad + thr * (direct + sf.emission); thr = thr * sf.albedo -- the integrator's own expressions and device functions.
 *   4. if sf is diffuse and ++diffuse == K the path ends in THE TAIL, without scattering: G = the look-up of the point record
 *      {sf.p, time, sf.n, bias} (sf.n the shaded normal, not flipped) by THE RULE of "Probe volumes", steps 1-6 in irradiance form, or
 *      with HRT_LIT_VISIBLE by that of "Probe visibility"; HRT_PROBE_EVAL_FACING is passed through; a degenerate point record gives
 *      G = 0.  value = (rad / 6.f) + thr * G per channel.
 *   5. otherwise the path scatters as the integrator does (the bounce segment's flags are the launch's) and remaining decreases;
 *      at 0 the path ends with value = rad / 6.f and no tail.
 *   6. samples in ascending order: sum = 0.f (or d_out on entry, under HRT_RADIANCE_ACCUMULATE), sum = sum + value; the output is
 *      sum / (float)n_samples, or the running sum.
 * PRUNING: hrt_trace_radiance drops work that cannot change a bit of its result (a last segment that cannot reach an emitter, a
 * path whose throughput is zero).  The kernels here drop nothing: the first would lose a hit at which the tail fires, and a tail
 * record counts its segments by the rule as written.
 * hrt_trace_lit_paths: hrt_trace_lit with tail_after -- the same records, keys, flags, eval_flags, bias, output and stream; one lane
 * of the device per ray.  On a ray whose first hit is diffuse, or that misses, tail_after = 1 gives hrt_trace_lit's bits.
 * hrt_path_tails: ONE sample per call (as hrt_camera_rays and hrt_probe_rays are per sample) and no volume: the end of the path of
 * every ray as a TAIL RECORD of HRT_TAIL_FLOATS = 16 floats at d_out[16i .. 16i+15] (device, 16-byte aligned):
 *     [0..7]   the point record {p, time, n, bias} of step 4, exactly what hrt_probe_eval* accepts;
 *     [8..10]  thr at the tail;
 *     [11]     a uint32 word: bits 0..7 the segments traced (1 .. 6), bit 31 set when the tail was reached;
 *     [12..14] a = rad / 6.f;
 *     [15]     0.
 *   A path that ends without a tail writes p = 0, n = 0, thr = 0 (a degenerate point record: its look-up gives 0); a degenerate
 *   ray writes 16 zeros.  CONTRACT B: for every K, the value of step 4 or 5 is a where bit 31 is clear and a + thr * G elsewhere,
 *   with G = hrt_probe_eval* (or _visible) of [0..7] -- hrt_trace_lit_paths gives exactly those bits.  `flags`: HRT_FLAG_EXACT_ONLY,
 *   HRT_FLAG_MESH_BRUTE (with EXACT_ONLY), HRT_FLAG_NO_LDS_TREE, HRT_RAYS_NORMALIZE.
 * hrt_probes_lit_paths_device / hrt_probes_lit_paths: hrt_probes_lit_device / hrt_probes_lit with tail_after: one wave of the device
 * per (probe, block of HRT_PROBE_BLOCK samples), the sum, the second launch, the scratch buffer, the LIMIT and the CONCURRENCY note
 * of "Lit rays".  CONTRACT A holds with hrt_trace_lit_paths (the same tail_after) in place of hrt_trace_lit.
 * Checked in this order, HRT_ERR_INVALID with hrt_last_error() naming the entry point and the culprit: flags; tail_after outside
 * 1 .. HRT_MAXBOUNCES; then for the three entry points with a volume everything "Lit rays" checks after the flags, in its order; for
 * hrt_path_tails a bias that is not finite; (n == 0 returns HRT_OK here and launches nothing;) d_rays NULL or not 16-byte aligned,
 * d_keys not 4-byte aligned, d_out NULL or not 16-byte aligned, n > 2^31 - 1; then a NULL scene and the library state.
 * OUT OF SCOPE (DESIGN.md section 5 "Lit paths"): the cooperative look-up, parking the lanes whose tail fires, probes that move,
 * multi-GPU; lens-camera sources with a tail are not in this section but in "Lit frames" below. */
#define HRT_TAIL_FLOATS 16u               /* floats of a tail record */
#define HRT_TAIL_REACHED 0x80000000u      /* word [11] of a tail record: the tail was reached */
HRT_API int hrt_trace_lit_paths(hrt_scene *scene, const hrt_probe_volume *volume, const float *d_rays, const uint32_t *d_keys, uint32_t n,
                                uint32_t first_sample, uint32_t n_samples, uint64_t seed, uint32_t flags, uint32_t eval_flags, float bias,
                                uint32_t tail_after, float *d_out, void *stream);
HRT_API int hrt_path_tails(hrt_scene *scene, const float *d_rays, const uint32_t *d_keys, uint32_t n, uint32_t sample, uint64_t seed,
                           uint32_t flags, float bias, uint32_t tail_after, float *d_out, void *stream);
HRT_API int hrt_probes_lit_paths_device(hrt_scene *scene, const hrt_probe_volume *volume, const float *d_probes, const uint32_t *d_keys, uint32_t n,
                                        uint32_t first_sample, uint32_t n_samples, uint64_t seed, uint32_t flags, uint32_t eval_flags, float bias,
                                        uint32_t tail_after, float *d_out, void *stream);
HRT_API int hrt_probes_lit_paths(hrt_scene *scene, const hrt_probe_volume *volume, const float *probes, const uint32_t *keys, uint32_t n,
                                 uint32_t spp, uint64_t seed, uint32_t flags, uint32_t eval_flags, float bias, uint32_t tail_after, float *out,
                                 hrt_stats *stats /* may be NULL */);

/* ---- Lit frames: the frame of a lens camera whose paths END in a probe volume -- "Lens cameras" in front of "Lit rays" or "Lit
 * paths", fused: one launch for all samples of a frame, no w*h*32-byte ray buffer, any projection, and a batch form.
 * THE RULE.  Sample s of pixel p = y*w + x is the value that hrt_trace_lit (tail_after == 0) or hrt_trace_lit_paths (tail_after in
 * 1 .. HRT_MAXBOUNCES) gives for record p of hrt_lens_rays(lens, w, h, s, seed), called with d_keys = NULL (key p), first_sample = s,
 * n_samples = 1 and the same seed, flags, eval_flags and bias.  The frame is the sum of those values in ascending sample order,
 * sum = 0.f (or d_frame on entry, under HRT_RADIANCE_ACCUMULATE), sum = sum + value, divided by (float)n_samples -- or the running
 * sums.  HRT_FLAG_GAMMA is applied after the division, as in lens frames.  A DEGENERATE sample (a fisheye pixel outside the circle,
 * a thin lens with c <= 0: see "Lens cameras") adds nothing and still counts in the divisor.  All arithmetic is fp32 without fused
 * multiply-add; every bit is the composition's.
 * hrt_render_lit_device: d_frame (device, h*w*3 floats, row-major) receives the means over samples [first_sample, first_sample +
 * n_samples), or with HRT_RADIANCE_ACCUMULATE the running sums.  Asynchronous on `stream`; touches none of the scene's per-launch
 * state and only READS the volume (the CONCURRENCY note of "Lit rays").  `flags` are hrt_render_lens_device's, refused by the same
 * names and texts: HRT_FLAG_EXACT_ONLY, HRT_FLAG_MESH_BRUTE (with EXACT_ONLY), HRT_FLAG_NO_LDS_TREE, HRT_RADIANCE_ACCUMULATE,
 * HRT_FLAG_GAMMA (not with ACCUMULATE).  `eval_flags` and `bias` are hrt_trace_lit's: HRT_PROBE_EVAL_FACING, HRT_LIT_VISIBLE (the
 * volume needs its depth moments).  With PERSPECTIVE and aperture_radius == 0 the frame is hrt_camera_rays + hrt_trace_lit[_paths]
 * per sample, bit for bit.
 * hrt_render_lit: the same into a HOST buffer, blocking, samples [0, spp); stats as hrt_render_lens (samples = w*h*spp).
 * HRT_RADIANCE_ACCUMULATE is refused (the sums live on the device).
 * hrt_render_lit_views_device / hrt_render_lit_views: the batch, laid out, keyed and staged as "Batched lens views" (its
 * CONCURRENCY note and LIMIT hold; `views` is hrt_lens_view, unchanged).  CONTRACT: frame v is bit-identical to
 * hrt_render_lit_device(scene, volume, &views[v].lens, w, h, first_sample, n_samples, views[v].seed, ...).  Stats count n_views * w *
 * h * spp samples; n_views == 0 zeroes them.
 * Checked in this order, HRT_ERR_INVALID with hrt_last_error() naming the entry point and the culprit: (the blocking forms:
 * HRT_RADIANCE_ACCUMULATE;) flags; the lens, as hrt_lens_rays checks it -- for a batch (an empty one skips to tail_after) views
 * NULL, then every lens, the message prefixed "views[<index>].lens"; the frame; n_samples == 0; first_sample + n_samples > 2^32; the
 * output NULL or not 4-byte aligned; for a batch the limit; tail_after > HRT_MAXBOUNCES; (n_views == 0 returns HRT_OK here and
 * launches nothing;) eval_flags, the volume and the bias in the order of "Lit rays"; then a NULL scene, a volume that lives on
 * another device than the scene, and the library state.
 * OUT OF SCOPE (DESIGN.md section 5 "Lit frames"): adaptive lit frames (the tile-list source), lit feature buffers, the cooperative
 * or parked look-up, probes that move, the streaming kernel, multi-GPU. */
HRT_API int hrt_render_lit_device(hrt_scene *scene, const hrt_probe_volume *volume, const hrt_lens *lens, uint32_t w, uint32_t h,
                                  uint32_t first_sample, uint32_t n_samples, uint64_t seed, uint32_t flags, uint32_t eval_flags, float bias,
                                  uint32_t tail_after, float *d_frame, void *stream);
HRT_API int hrt_render_lit(hrt_scene *scene, const hrt_probe_volume *volume, const hrt_lens *lens, uint32_t w, uint32_t h, uint32_t spp,
                           uint64_t seed, uint32_t flags, uint32_t eval_flags, float bias, uint32_t tail_after, float *out_rgb,
                           hrt_stats *stats /* may be NULL */);
HRT_API int hrt_render_lit_views_device(hrt_scene *scene, const hrt_probe_volume *volume, const hrt_lens_view *views, uint32_t n_views,
                                        uint32_t w, uint32_t h, uint32_t first_sample, uint32_t n_samples, uint32_t flags, uint32_t eval_flags,
                                        float bias, uint32_t tail_after, float *d_frames, void *stream);
HRT_API int hrt_render_lit_views(hrt_scene *scene, const hrt_probe_volume *volume, const hrt_lens_view *views, uint32_t n_views, uint32_t w,
                                 uint32_t h, uint32_t spp, uint32_t flags, uint32_t eval_flags, float bias, uint32_t tail_after,
                                 float *out_rgb, hrt_stats *stats /* may be NULL */);

/* ---- Lit bakes: the FINAL GATHER of a baked-lighting pipeline -- "Baking" in front of "Lit rays" or "Lit paths", fused: the
 * cosine-weighted rays of bake points whose paths END in a probe volume, one launch for all samples, no n*32-byte ray buffer.  The
 * texel keeps its own contact shadows and direct light; everything beyond the hit (or the K-th diffuse hit) is read from the volume.
 * THE RULE.  Sample s of point i is the value that hrt_trace_lit (tail_after == 0) or hrt_trace_lit_paths (tail_after in
 * 1 .. HRT_MAXBOUNCES) gives for record i of hrt_bake_rays(d_points, d_keys, n, s, seed), called with the same d_keys, first_sample = s,
 * n_samples = 1 and the same seed, flags, eval_flags and bias.  The output is the sum of those values in ascending sample order,
 * sum = 0.f (or d_out on entry, under HRT_RADIANCE_ACCUMULATE), sum = sum + value, divided by (float)n_samples -- or the running
 * sums.  A DEGENERATE sample (what "Baking" calls degenerate: its bake ray record has direction 0) adds nothing and still counts in
 * the divisor: a degenerate point gives 0 in mean mode and leaves its sums as they are under HRT_RADIANCE_ACCUMULATE.  All
 * arithmetic is fp32 without fused multiply-add; every bit is the composition's.
 * BIAS: `bias` is the look-up's bias of "Lit rays", applied at the HIT where the path ends in the volume.  It is NOT the point
 * record's own bias float (record[7]), which the rule of "Baking" adds to the ray's ORIGIN along the point's normal; the two are
 * independent and neither replaces the other.
 * UNITS: hrt_bake's (the mean over samples of radiance / 6; the irradiance at the point is pi times the mean radiance; NO factor
 * is applied), so the result is directly comparable with hrt_bake and with hrt_probe_eval (irradiance form) on the same records.
 * hrt_bake_lit_device: 3 floats per point at d_out[3i .. 3i+2], the means over samples [first_sample, first_sample + n_samples), or
 * with HRT_RADIANCE_ACCUMULATE the running sums.  Asynchronous on `stream`; touches none of the scene's per-launch state and only
 * READS the volume (the CONCURRENCY note of "Lit rays").  `flags` are hrt_bake_device's, refused by the same names and texts:
 * HRT_FLAG_EXACT_ONLY, HRT_FLAG_MESH_BRUTE (with EXACT_ONLY), HRT_FLAG_NO_LDS_TREE, HRT_RADIANCE_ACCUMULATE.  `eval_flags` are
 * hrt_trace_lit's: HRT_PROBE_EVAL_FACING, HRT_LIT_VISIBLE (the volume needs its depth moments).
 * hrt_bake_lit: the same from and into HOST buffers (`points`, `keys`, `out`; 4-byte aligned), blocking, samples [0, spp); stats as
 * hrt_bake (samples = n * spp; n == 0 zeroes them).  HRT_RADIANCE_ACCUMULATE is refused (the sums live on the device).
 * Checked in this order, HRT_ERR_INVALID with hrt_last_error() naming the entry point and the culprit: (the blocking form:
 * HRT_RADIANCE_ACCUMULATE;) flags; (n == 0 returns HRT_OK here and launches nothing;) the points NULL or misaligned (device 16
 * bytes, host 4); the keys not 4-byte aligned; n > 2^31 - 1; n_samples == 0; first_sample + n_samples > 2^32; the output NULL or
 * not 4-byte aligned; tail_after > HRT_MAXBOUNCES; eval_flags, the volume and the bias in the order of "Lit rays"; then a NULL
 * scene, a volume that lives on another device than the scene, and the library state.
 * OUT OF SCOPE (DESIGN.md section 5 "Lit bakes"): the cooperative or parked look-up, batched point sets over several volumes,
 * multi-GPU. */
HRT_API int hrt_bake_lit_device(hrt_scene *scene, const hrt_probe_volume *volume, const float *d_points, const uint32_t *d_keys, uint32_t n,
                                uint32_t first_sample, uint32_t n_samples, uint64_t seed, uint32_t flags, uint32_t eval_flags, float bias,
                                uint32_t tail_after, float *d_out, void *stream);
HRT_API int hrt_bake_lit(hrt_scene *scene, const hrt_probe_volume *volume, const float *points, const uint32_t *keys, uint32_t n, uint32_t spp,
                         uint64_t seed, uint32_t flags, uint32_t eval_flags, float bias, uint32_t tail_after, float *out,
                         hrt_stats *stats /* may be NULL */);

/* ---- Adaptive lit frames: the per-tile sample counts of hrt_render_adaptive for a lit frame -- "Adaptive lens frames" with the
 * sums of "Lit frames".  A lit frame is noise-free but for direct-light penumbrae, lens blur and edges: most tiles stop at min_spp.
 * The rounds, the estimate and the counts are EXACTLY the rule stated at hrt_render_adaptive, with the sums of hrt_render_lit in
 * place of hrt_render's: round 0 adds samples [0, min_spp/2) to every HRT_TILE x HRT_TILE tile, round 1 adds [min_spp/2, min_spp) and
 * judges every tile, every later round adds min(n, max_spp - n) samples to the tiles still active and judges them, until none is
 * active.  Every round is one launch of a fused lit kernel over the list of active tiles (one lane per pixel of a listed tile),
 * adding its samples in sample order onto the stored sums.  A DEGENERATE sample (see "Lit frames") adds nothing and counts in the
 * divisor; a tile of a fisheye frame wholly outside the image circle has tile_err 0, stops at min_spp and is all zeros.
 * CONTRACT A: every tile of the result is bit-identical to the same tile of hrt_render_lit(volume, lens, w, h, count of that tile,
 * seed, flags, eval_flags, bias, tail_after), for every projection, both tail rules (tail_after == 0 and 1 .. HRT_MAXBOUNCES), every
 * look-up (HRT_PROBE_EVAL_FACING, HRT_LIT_VISIBLE) and every permitted flag set, HRT_FLAG_GAMMA included.
 * hrt_render_lit_adaptive_device: d_frame (device, h*w*3 floats, ROW-MAJOR) receives the means (gamma-corrected with
 * HRT_FLAG_GAMMA), d_tile_spp (device, may be NULL) tiles_y * tiles_x uint32 counts, row-major.  Runs on `stream` and synchronises
 * it once per round from round 1 on, as hrt_render_lens_adaptive_device does; a fault while a round runs ends the call with
 * HRT_ERR_DEVICE at that round's synchronisation.
 * hrt_render_lit_adaptive: the same into HOST buffers out_rgb[h*w*3] and out_tile_spp (may be NULL), blocking.  stats (may be NULL)
 * as hrt_render_lens_adaptive: kernel_ms = the lit kernels' time summed over all rounds, samples = sum over in-image pixels of their
 * tile's count (degenerate samples count).
 * FLAGS: hrt_render_lens_adaptive's, refused by the same names and texts.  `eval_flags`, `bias` and `tail_after` are hrt_render_lit's.
 * Checked in this order, HRT_ERR_INVALID with hrt_last_error() naming the entry point and the culprit: everything
 * hrt_render_lens_adaptive checks before the scene, in its order (flags; params; the lens; the frame; the LIMIT; the output
 * pointers); tail_after > HRT_MAXBOUNCES; eval_flags, the volume and the bias in the order of "Lit rays"; then a NULL scene, a
 * volume that lives on another device than the scene, and the library state.
 * CONCURRENCY: the call shares the tile-major sums and the round scratch with hrt_render_adaptive and hrt_render_lens_adaptive: it
 * may NOT overlap another adaptive call of the same scene, lit, lens or pinhole.  Nothing of the trace launches' state is touched:
 * it may overlap a plain render or a query of the same scene on another stream.  It only READS the volume (the CONCURRENCY note of
 * "Lit rays").
 * OUT OF SCOPE (DESIGN.md section 5 "Adaptive lit frames"): batched views (hrt_render_lit_views stays uniform), rank
 * partitions, denoising of adaptive frames, the streaming kernel, multi-GPU. */
HRT_API int hrt_render_lit_adaptive_device(hrt_scene *scene, const hrt_probe_volume *volume, const hrt_lens *lens, uint32_t w, uint32_t h,
                                           const hrt_adaptive *params, uint64_t seed, uint32_t flags, uint32_t eval_flags, float bias,
                                           uint32_t tail_after, float *d_frame, uint32_t *d_tile_spp /* may be NULL */, void *stream);
HRT_API int hrt_render_lit_adaptive(hrt_scene *scene, const hrt_probe_volume *volume, const hrt_lens *lens, uint32_t w, uint32_t h,
                                    const hrt_adaptive *params, uint64_t seed, uint32_t flags, uint32_t eval_flags, float bias,
                                    uint32_t tail_after, float *out_rgb, uint32_t *out_tile_spp /* may be NULL */,
                                    hrt_stats *stats /* may be NULL */);

/* ---- Path features: the denoisers' feature record taken at the FIRST DIFFUSE hit of the integrator's own path.  The features of
 * "denoising" above are first-hit features: on a mirror or a glass sphere they carry the mirror's own flat albedo and smooth normal,
 * so the filter sees no edge inside a reflection and blurs what the mirror shows.  Here mirror and glass are followed: the albedo is
 * the path's throughput at its first diffuse hit (the factor by which everything beyond that hit reaches the pixel, which is what
 * the filter demodulates by), the normal is that surface's, the emission is what the path met on the way, the depth is the length
 * of the chain.  It is "Lit paths" with K = 1 and a feature record for a tail record: the same hook of the same kernel body.
 * THE RULE (tests/path_features_ref.py states the fold again in NumPy).  All arithmetic is fp32 without fused multiply-add, in the
 * order written.  A PATH-FEATURE RECORD of one sample is HRT_FEATURE_FLOATS = 12 floats in the layout of hrt_render_features.  For
 * a ray {o, time, d, tmax} (tmax is not read), key k and sample s:
 *   1. the path starts as a path of hrt_path_tails starts: stream (seed, k, s) with the draw index set to 3, the filter margin and
 *      far-origin rule of a first segment, the same DEGENERATE rays, which give 12 zeros; thr = 1, E = 0, depth = 0.f, remaining = 6.
 *   2. per segment: h = the closest hit, meshes included.  A miss ends the path UNREACHED.
 *   3. a hit: sf = the shaded surface.  In a scene with lights the direct light at sf is drawn as the integrator draws it, because
 *      its draws move the stream; its value is not used.  Then, in this order: E = E + thr * sf.emission; depth = depth + h.t;
 *      thr = thr * sf.albedo.
 *   4. if sf is diffuse the path ends REACHED, without scattering.  Otherwise it scatters as the integrator does (the bounce
 *      segment's flags are the launch's) and remaining decreases; at 0 the path ends unreached.  Nothing is pruned.
 *   5. the record:             [0..2]    [3..5]                           [6..8]  [9]     [10]  [11]
 *        reached               thr       sf.n (shaded, not flipped)       E       depth   1.f   0
 *        unreached             0, 0, 0   0, 0, 0                          E       0       0     0
 *      An unreached path keeps E, the emitters seen on the way.  The sky is NOT added; a first-hit miss adds nothing either.
 * THE FRAME FORM: per pixel, feature = (sum of the records of samples [first_sample, first_sample + n_samples) in ascending order,
 * in fp32, starting from +0) / (float)n_samples.  The ray of sample s is the one hrt_lens_rays writes for it, the key is the pixel
 * index y*w + x.  A sample the lens does not trace (outside a fisheye's circle) adds nothing and counts in the divisor.
 * n_samples == 0 is REFUSED: hrt_render_features' pixel-centre ray has no stream to scatter with.
 * CONTRACT A: a sample whose first segment misses, or whose first hit is diffuse, gives the first-hit values (1 * x, 0 + x and
 * 0 + 1 * x are exact), so a pixel all of whose samples are such has the bits of hrt_render_lens_features and, for a pinhole, of
 * hrt_render_features.
 * CONTRACT B: the record agrees with the tail record of hrt_path_tails(tail_after = 1, bias = 0) for the same ray, key, sample, seed
 * and flags: [3..5] = tail [4..6], [0..2] = tail [8..10], [10] = bit 31 of the tail's word (as 1.f or 0), and in a scene without
 * lights E / 6.f = tail [12..14] on every path that does not end in a miss under a sky (there the tail record adds the sky; E
 * does not).
 * CONTRACT C: the frame entry points are the fold above over hrt_lens_rays and hrt_path_features, sample by sample; frame v of a
 * batch is the single frame of views[v].lens with seed views[v].seed.
 * hrt_path_features: ONE sample per call, as hrt_path_tails: record i at d_out[12i .. 12i+11] (device, 4-byte aligned).  One lane
 * of the device per ray, asynchronous on `stream`; touches none of the scene's per-launch state.  `flags`: HRT_FLAG_EXACT_ONLY,
 * HRT_FLAG_MESH_BRUTE (with EXACT_ONLY), HRT_FLAG_NO_LDS_TREE, HRT_RAYS_NORMALIZE.  Checked in this order, HRT_ERR_INVALID with
 * hrt_last_error() naming the entry point and the culprit: flags; (n == 0 returns HRT_OK here and launches nothing;) d_rays NULL or
 * not 16-byte aligned, d_keys not 4-byte aligned, d_out NULL or not 4-byte aligned, n > 2^31 - 1; then a NULL scene and the library
 * state.
 * hrt_render_lens_path_features: the frame form for a lens, d_features (device) h*w*HRT_FEATURE_FLOATS floats, row-major, one lane
 * per pixel, no ray buffer; asynchronous on `stream`, and like hrt_render_lens_features no part of the ordering of the scene's
 * feature launches.  Checked in the order of hrt_render_lens_features: the lens; the frame; n_samples == 0; first_sample + n_samples
 * > 2^32 - 1; d_features NULL or not 4-byte aligned; then a NULL scene.
 * hrt_render_path_features: the same through the pinhole lens of `cam` (PERSPECTIVE, aperture 0).  Checked in the order of
 * hrt_render_features: cam NULL; the frame; n_samples == 0; the sample range; d_features; the scene; then the camera's values.
 * hrt_render_lens_views_path_features: the batch, n_views * h * w * HRT_FEATURE_FLOATS floats, view-major; the table, the
 * CONCURRENCY note and the LIMIT (2^31 / 16 items) of hrt_render_lens_views_features.  Checked in its order: (n_views == 0 returns
 * HRT_OK and launches nothing;) views NULL; every lens; the frame; n_samples == 0; the sample range; d_features NULL or not 4-byte
 * aligned; the limit; then a NULL scene.
 * GUIDED RENDERS: hrt_render_denoised_guides and hrt_render_denoised_var_guides are hrt_render_denoised and
 * hrt_render_denoised_var with one parameter more, where the features come from.  HRT_GUIDES_FIRST_HIT gives the bits of the
 * existing functions; HRT_GUIDES_FIRST_DIFFUSE takes the features of samples [0, feature_spp) from hrt_render_path_features and
 * requires feature_spp >= 1: the result is bit-identical to hrt_denoise / hrt_denoise_var of the same frames with
 * hrt_render_path_features(0, feature_spp).  Checked after the parameters, the frame and spp, and before feature_spp > spp: any
 * other value of `guides`, then feature_spp == 0 with HRT_GUIDES_FIRST_DIFFUSE, each refused by name.  Every existing entry point
 * keeps its signature and its bits.
 * OUT OF SCOPE (DESIGN.md section 5 "Path features"): pixel-centre paths; temporal accumulation with path guides (hrt_render_temporal
 * reprojects with the first-hit depth, which a path depth is not); a virtual (mirrored) normal; K > 1; adaptive frames. */
#define HRT_GUIDES_FIRST_HIT 0u           /* guides: the features of hrt_render_features */
#define HRT_GUIDES_FIRST_DIFFUSE 1u       /* guides: the features of hrt_render_path_features */
HRT_API int hrt_path_features(hrt_scene *scene, const float *d_rays, const uint32_t *d_keys, uint32_t n, uint32_t sample, uint64_t seed,
                              uint32_t flags, float *d_out, void *stream);
HRT_API int hrt_render_path_features(hrt_scene *scene, const hrt_camera *cam, uint32_t w, uint32_t h, uint32_t first_sample, uint32_t n_samples,
                                     uint64_t seed, float *d_features, void *stream);
HRT_API int hrt_render_lens_path_features(hrt_scene *scene, const hrt_lens *lens, uint32_t w, uint32_t h, uint32_t first_sample,
                                          uint32_t n_samples, uint64_t seed, float *d_features, void *stream);
HRT_API int hrt_render_lens_views_path_features(hrt_scene *scene, const hrt_lens_view *views, uint32_t n_views, uint32_t w, uint32_t h,
                                                uint32_t first_sample, uint32_t n_samples, float *d_features, void *stream);
HRT_API int hrt_render_denoised_guides(hrt_scene *scene, const hrt_camera *cam, uint32_t w, uint32_t h, uint32_t spp, uint32_t feature_spp,
                                       uint64_t seed, uint32_t flags, uint32_t guides, const hrt_denoise_params *p, float *out_rgb,
                                       hrt_stats *stats /* may be NULL */);
HRT_API int hrt_render_denoised_var_guides(hrt_scene *scene, const hrt_camera *cam, uint32_t w, uint32_t h, uint32_t spp, uint32_t feature_spp,
                                           uint64_t seed, uint32_t flags, uint32_t guides, const hrt_denoise_var_params *p, float *out_rgb,
                                           float *out_variance /* may be NULL */, hrt_stats *stats /* may be NULL */);

/* The PPM file of main.cpp:252-262 encoded ON THE DEVICE from a row-major frame (device, h*w*3 floats).
 * format 3: the reference's ASCII file byte for byte ("P3\n<w> <h>\n255\n", then "r g b " per pixel, "\n");
 * format 6: the same integers as bytes (binary PPM; negative values, which P3 prints with a sign, clamp to 0).
 * d_out: device buffer of `capacity` bytes (16*w*h + 64 always suffices for non-negative frames; the call
 * fails with the needed size otherwise); *bytes = size of the file.  Synchronises the stream. */
HRT_API int hrt_encode_ppm(const float *d_frame, uint32_t w, uint32_t h, int format, unsigned char *d_out,
                   size_t capacity, size_t *bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HRT_H */
