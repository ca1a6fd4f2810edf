// pt_launch.h -- host-callable launchers of the kernels in pt_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "prt.h"
#include "prt_types.h"
#include "pt_layout.h"

namespace prt {

// launcher-level choices of a context (prt_set_option / PRT_WAVES, PRT_SCATTER, PRT_GENERIC): what is forced, for tests and experiments
struct LaunchOpts {
    int waves = 0;          // 0: chosen per launch; 5 / 6: that build of the kernel (waves per SIMD the register allocator leaves room for)
    int scatter = -1;       // -1: chosen per launch; 0: one 8x8 tile per wave; 1: a wave's pixels scattered over the launch's tiles
    int generic = 0;        // 1: the run-time-dispatched material set even where the scene's own set is compiled
    int any_dist = 0;       // 1: the set's instance that carries every microfacet distribution even where the scene uses one (PT_MATS_DISTS)
    int pix_per_wave = 0;   // 0: chosen per launch; 64 / 32 / 16: pixels a wave renders (FrameArgs::sub_shift)
    int pool = 0;           // 1: render_kernel_pool (pt_pool.h: shading waves + walker waves around a pool of parked contexts) where a launch can take it
};
// what a launch ran: kernel variant, wave-count build, pixel-to-wave mapping (prt_kernel_variant)
struct RenderLaunch { const char* name = ""; int waves = 0; int scatter = 0; int ordered = 0; int pool = 0; int pix_per_wave = 64; int adaptive = 0; int list = 0; };   // ordered: the tiles were taken in the launcher's order; adaptive: the PT_MATS_ADAPT build, list: over a live-pixel list

// a tree beyond one XCD's L2 (more than 64 k node pairs): what the launchers and the render drivers choose by tree size, they choose by this
inline bool big_tree(const DevScene& sc) { return sc.n_pairs > 65536u; }

// launches the row of the variant table the scene and the options select (pt_variant.h select_variant)
RenderLaunch launch_render(const DevScene& sc, const DevCamera& cam, const DevState& S, const FrameArgs& fa, float4* fb,
                           hipStream_t stream, const LaunchOpts& lo);

// workgroups (tiles) launch_render uses for a width x rows frame part
unsigned render_tile_count(int width, int rows);
#ifdef PT_POOL_STATS
void dump_pool_stats();                   // development builds: what the waves of the pool kernel did (pt_pool.h)
#endif
#ifdef PT_PHASE_CLOCKS
void dump_phase_clocks();                 // development builds: prints the per-phase cycle shares of all launches so far
#endif
// per-camera part of createCamRay (camera.cl:19-28), on the host with the arithmetic of pt_device.h
void make_dev_camera(const prt_camera& in, DevCamera& out);
void launch_state_to_rtd(const DevState& S, prt_path_state* out, size_t n, hipStream_t stream);
void launch_rtd_to_state(const prt_path_state* in, const DevState& S, float4* fb, size_t n, hipStream_t stream);
void launch_selftest_math(int fn, const float* a, const float* b, float* out, int n, hipStream_t stream);
void launch_selftest_fn(int fn, const float* params, const float* in, float* out, int n, hipStream_t stream);
// prt_selftest_fn fn 13 / 14 (pt_selftest.h selftest_env): env_sample / env_pdf and env_lookup on a map with its build_env_cdf tables (device pointers)
void launch_selftest_env(int fn, const float* env, int env_w, int env_h, const float* rows, const float* cols, const float* in, float* out, int n, hipStream_t stream);
// prt_selftest_fn fn 12 (pt_filter.hip): filter_offset of pt_filter.h on the device, n cases of 32 floats in / out (in: gx, gy, k as uint bits;
// out: dx, dy); tab: the kind's table (device) or null
void launch_selftest_filter(unsigned kind, float r, const float* tab, const float* in, float* out, int n, hipStream_t stream);
// the Gaussian and Blackman-Harris kinds' table T[0 .. PT_FILTER_TAB] of radius r (prt.h prt_set_pixel_filter; host, float64 rounded to f32)
void build_filter_table(unsigned kind, float r, float* tab);
void launch_tonemap(const float4* fb, unsigned char* out, const FrameArgs& fa, hipStream_t stream);
void launch_count(const DevState& S, size_t n, unsigned spp, unsigned long long* out3, hipStream_t stream);
// prt_render_adaptive: the local ids of the n-pixel frame's pixels that the adaptive freeze rule (max_spp, DevState::q4.w bit 31) has not frozen,
// in increasing order, into list; their number into *count (device).  wave_off: ceil(n / 64) words of scratch
void launch_live_list(const DevState& S, size_t n, unsigned max_spp, uint32_t* wave_off, uint32_t* list, uint32_t* count, hipStream_t stream);
// pt_denoise.hip.  prt_render_guides: `samples` guide samples per pixel of the frame part of `fa` into out (2 float4 per pixel: {albedo, coverage},
// {normal, depth}).  tri_prev non-null: a triangle snapshot is pending -- the triangle records (one per slot, as sc.tri_geom) of the geometry
// before the update(s); prims non-null: a primitive snapshot is pending (prt.h prt_update_primitives) -- the sphere / SDF / quad tables before
// the update(s) (pt_prims.h).  With either, the motion instances of the guide kernels, which also write the motion plane (prt.h
// prt_set_motion; one float4 {D, m} per pixel); the two snapshots are independent, and without both `motion` is not written
struct PrimPrev;
void launch_guides(const DevScene& sc, const DevCamera& cam, const FrameArgs& fa, unsigned samples, float4* out, const TriGeom* tri_prev,
                   const PrimPrev* prims, float4* motion, hipStream_t stream);
// the W x H planes of one filter call (prt_denoise and its temporal and record variants): the framebuffer {c, alpha}, the guides (2 float4
// per pixel), two ping-pong planes of {rgb, v}, the Gaussian of v, and the filtered rgba (alpha of fb).  All device memory; the record calls
// write fb and guides themselves (VarianceSource)
struct FilterPlanes { float4* fb; float4* guides; float4* buf0; float4* buf1; float* g; float4* out; int W, H; };
// what the variance step takes the frame's {rgb, v} from.  records (W x H records of prt.h, device): rec_import_kernel, which also writes
// planes.fb and planes.guides, and 1 into *no_stats if any record has has_stats != 1 (the caller zeroes the word first).  Otherwise planes.fb
// as it stands: spatial, the 5x5 moments of its luminance, else the stats plane adapt with the path counts q4
struct VarianceSource {
    bool spatial = false; const uint4* q4 = nullptr; const float2* adapt = nullptr;
    const float4* records = nullptr; unsigned* no_stats = nullptr;
};
// the variance step: {rgb, v} of the frame to where launch_filter_chain, called with (temporal) or without temporal parameters, reads it
void launch_filter_variance(const FilterPlanes& planes, bool temporal, const VarianceSource& src, hipStream_t stream);
// pt_temporal.hip.  prt_denoise_temporal: the previous call's history (read) and the halves this call writes; `valid` false = empty history
struct TemporalHistory {
    const float4* cn_prev;          // {c.rgb, n} per pixel
    const float4* m_prev;           // {m1, m2, v, 0}
    const float4* guides_prev;      // the guides of the previous call (2 float4 per pixel)
    DevCamera cam_prev;
    bool valid;
    float4* cn;                     // written by this call
    float4* m;
    // prt_set_temporal_response: the fast history {f.rgb, took the history branch} of the previous call (read) and of this one (written),
    // and the setting.  fast null = off: today's reprojection alone, and none of the others is read
    const float4* fast_prev = nullptr;
    float4* fast = nullptr;
    uint32_t fast_cap = 0, radius = 0;
    float k = 0.0f;
};
// everything behind the variance step.  t null: (gauss, a-trous) x p.passes, ping-pong between buf0 and buf1, the last pass into planes.out
// with the framebuffer's alpha.  t non-null (cam and h with it; motion: null, or the motion plane of the guides, W x H float4 {D, m}): the
// reprojection in front, the clamp behind it if h->fast is set, and under PRT_TEMPORAL_FEEDBACK_ATROUS pass 0's colour into h->cn
void launch_filter_chain(const FilterPlanes& planes, const prt_denoise_params& p, const prt_temporal_params* t, const DevCamera* cam,
                         const TemporalHistory* h, const float4* motion, hipStream_t stream);
// ... its temporal steps (the kernels of pt_temporal.hip, for the chain alone): the reprojection of `var` ({rgb, v} of the frame) into `in`
// (the passes' input) and the new history, then the clamp; and the feedback of pass 0's output
void launch_temporal_front(const FilterPlanes& planes, const float4* var, float4* in, const prt_temporal_params& t, const DevCamera& cam,
                           const TemporalHistory& h, const float4* motion, hipStream_t stream);
void launch_temporal_feedback(const float4* pass0, int W, int H, float4* h_cn, hipStream_t stream);
// pt_records.hip.  prt_export_denoise_inputs: the records (prt.h: 4 float4 per pixel) of a W x rows frame part; adapt null = no stats
// (v = 0, has_stats = 0).  launch_records_import: VarianceSource::records, for launch_filter_variance alone -- var the plane of {c, v of the record}
void launch_records_export(const float4* fb, const uint4* q4, const float2* adapt, const float4* guides, int W, int rows, float4* records,
                           hipStream_t stream);
void launch_records_import(const float4* records, int W, int H, float4* fb, float4* guides, float4* var, unsigned* no_stats, hipStream_t stream);
// pt_refit.hip.  prt_update_vertices: the tables of the uploaded tree (PackedScene::slot_vtx, level_pairs: device; level_first: host)
struct RefitTables {
    const uint32_t* slot_vtx;       // device, n_slots
    size_t n_slots;
    const uint32_t* level_pairs;    // device, the pairs sorted by level
    const uint32_t* level_first;    // HOST, n_levels + 1: level l is level_pairs[level_first[l] .. level_first[l + 1])
    uint32_t n_levels;
    int root_is_leaf;
    uint32_t root_leaf_first, root_leaf_count;
};
// 1 into *flag (device; the caller zeroes it first) if x, y or z of any of the n_vertices float4 vertices is not finite
void launch_refit_check(const float* vertices, size_t n_vertices, uint32_t* flag, hipStream_t stream);
// the triangle records of every slot (normals null: tri_nrm is left alone), then the boxes level by level, deepest first, and the root's box
// into root6 (device, 6 floats)
void launch_refit(const RefitTables& t, const float* vertices, const float* normals, NodePair* pairs, TriGeom* tri_geom, TriNrm* tri_nrm,
                  float* root6, hipStream_t stream);
// pt_cost.hip.  prt_bvh_cost: the SAH cost of a tree with an inner root from its n_pairs >= 1 pairs (device), one launch per level of
// PT_COST_BLOCK-fold reduction; work: cost_work_doubles(n_pairs) doubles of scratch (device).  Returns where in `work` the cost is once the
// stream has run the launches
size_t cost_work_doubles(uint32_t n_pairs);
const double* launch_bvh_cost(const NodePair* pairs, uint32_t n_pairs, double* work, hipStream_t stream);
// ... of a tree whose root is a leaf of `count` triangles into work[0]: root6 the root's box on the device, or null: host_root6 (host, 6 floats)
void launch_bvh_cost_leaf_root(const float* root6, const float* host_root6, uint32_t count, double* work, hipStream_t stream);
// pt_prims.hip.  prt_update_primitives: `count` prt_mesh records (device, 16-byte aligned; n_spheres spheres, then n_sdfs SDF primitives, then
// quads) into the three tables, and 1 into *flag (device; the caller zeroes it first) if a record's t differs from types[i] or a field that
// is read is not finite
void launch_prims_pack(const void* meshes, uint32_t count, uint32_t n_spheres, uint32_t n_sdfs, const uint8_t* types, DevSphere* spheres,
                       DevSdf* sdfs, DevQuad* quads, uint32_t* flag, hipStream_t stream);
// pt_normals.hip.  prt_set_smooth_normals: the topology on the device and the face buffer (all device memory)
struct SmoothTables {
    const uint32_t* corner_group;   // 3 n_tris: the group of every corner
    const uint32_t* group_first;    // n_groups + 1: group g is member_face[group_first[g] .. group_first[g + 1])
    const uint32_t* member_face;    // 3 n_tris: the faces of the groups' corners, ascending corner order within a group
    void* face_f;                   // n_tris x 16 bytes {f, l}: written by the face kernel, gathered by the corner kernel
    void* face_r;                   // n_tris x 16 bytes {r, 0} for the area weighting, null for the unit weighting
    uint32_t n_tris;
    float crease_cos;
};
// the face records of `vertices`, then one normal per corner into `normals` (device, float4[3 n_tris], 16-byte aligned): two launches
void launch_smooth_normals(const SmoothTables& t, const float* vertices, float* normals, hipStream_t stream);
// pt_pose.hip.  prt_set_skin: the rest pose and the per-corner influences on the device (all device memory, 16-byte aligned)
struct PoseTables {
    const float* rest_v;            // float4[3 n_tris]
    const float* rest_n;            // float4[3 n_tris], or null: no normals are posed
    const uint16_t* bone_index;     // 4 per corner
    const float* bone_weight;       // 4 per corner
    uint32_t n_tris;
};
// the posed vertices into out_v and, with rest normals, the posed normals into out_n (device, float4[3 n_tris] each, 16-byte aligned) from
// `matrices` (device, 16-byte aligned, 12 floats per bone): one launch
void launch_pose(const PoseTables& t, const float* matrices, float* out_v, float* out_n, hipStream_t stream);
// pt_morph.hip.  prt_set_morph_targets: the base mesh and the per-corner table of the targets' entries on the device (all device memory,
// 16-byte aligned)
struct MorphTables {
    const float* base_v;            // float4[3 n_tris]
    const float* base_n;            // float4[3 n_tris], or null: no normals are morphed
    const uint32_t* offset;         // 3 n_tris + 1: corner c owns entries offset[c] .. offset[c + 1], in ascending target order
    const float* entry_p;           // float4 per entry: {dp.x, dp.y, dp.z, the target's number as bits}
    const float* entry_n;           // float4 per entry: dn (not read without base_n)
    uint32_t n_tris;
    // prt_set_morph_targets_layout with PRT_MORPH_LAYOUT_PLANES: `planes` is set, offset and the entries are null, and the table is per (block
    // of 64 corners, target) one plane (pt_morph.h): block b owns planes block_first[b] .. block_first[b + 1], in ascending target order
    bool planes = false;
    const uint32_t* block_first = nullptr;    // ceil(3 n_tris / 64) + 1
    const void* plane_head = nullptr;         // 16 bytes per plane: {target, 0, mask_lo, mask_hi}
    const float* plane_p = nullptr;           // float[3][64] per plane: the x, y and z rows of dp, +0 on unlisted lanes
    const float* plane_n = nullptr;           // the same for dn (not read without base_n)
};
// the morphed vertices into out_v and, with base normals, the morphed and renormalised normals into out_n (device, float4[3 n_tris] each,
// 16-byte aligned) from `weights` (device, one float per target): one launch
void launch_morph(const MorphTables& t, const float* weights, float* out_v, float* out_n, hipStream_t stream);
// the same morph, un-normalised and in registers, as the rest pose of the skin's pose (skin.rest_v and rest_n are not read): one launch
void launch_pose_morphed(const MorphTables& t, const PoseTables& skin, const float* matrices, const float* weights, float* out_v, float* out_n,
                         hipStream_t stream);
// pt_build.hip.  prt_rebuild_bvh: the scratch of one build over T triangles, carved out of one device allocation of the context
struct BuildNode;
struct BuildExtent;
struct BuildHeader;
struct BuildWork {
    uint64_t* keys; uint64_t* keys_sorted;              // T: code << 32 | triangle
    uint64_t* pair_keys; uint64_t* pair_keys_sorted;    // T - 1: depth << 32 | first position, per inner node of the radix tree
    BuildNode* nodes; uint32_t* parent;                 // T - 1
    uint32_t* order_in; uint32_t* order;                // T - 1: the inner node of each sorted position
    uint32_t* pair_of; uint32_t* leaf_tris; uint32_t* slot_base;      // T - 1
    uint32_t* old_slot;                                 // T: a slot of the tree being replaced that holds the triangle, or 0xFFFFFFFF
    float* partials; BuildExtent* extent;               // 6 floats per block of 256 triangles; the extent of the centres
    BuildHeader* hdr;                                   // what the host reads back
    uint32_t* flags;                                    // [0] a non-finite vertex, [1] a triangle without an old slot
    void* temp; size_t temp_bytes;                      // the sorts' and the scan's temporary storage
};
// the pointers of `w` for T triangles from `base` on (null: sizes only), the bytes all of it takes in *bytes
hipError_t build_work_layout(uint32_t T, void* base, BuildWork& w, size_t* bytes);
// w.old_slot from the slot table of the tree being replaced; check_missing: 1 into w.flags[1] (zeroed by the caller) if a triangle has none
void launch_build_old_slots(const BuildWork& w, const uint32_t* old_slot_vtx, size_t n_old_slots, uint32_t T, bool check_missing, hipStream_t stream);
// rules 1 - 7 of prt.h: NodePair::meta of every pair (boxes zeroed), slot_vtx (T entries), the identity level_pairs, and w.hdr.  T <= max_leaf:
// slot_vtx alone (a leaf root over slots 0 .. T - 1)
hipError_t launch_build_tree(const BuildWork& w, const float* vertices, uint32_t T, uint32_t max_leaf, NodePair* pairs, uint32_t* slot_vtx,
                             uint32_t* level_pairs, hipStream_t stream);
// per new slot: TriNrm from the triangle's old slot (carry_nrm) and the motion snapshot in the new slot order (prev_new non-null; pt_build.h)
void launch_build_carry(const BuildWork& w, const uint32_t* slot_vtx, uint32_t n_slots, bool carry_nrm, const TriNrm* nrm_old, TriNrm* nrm_new,
                        const TriGeom* prev_old, const TriGeom* geom_new, TriGeom* prev_new, hipStream_t stream);
// pt_cast.hip.  prt_cast_rays / prt_occluded: n prt_ray records (device, 16-byte aligned) through the scene; any_hit false: one prt_hit per
// ray into out (48 bytes each, 16-byte aligned), true: one uint32 per ray.  slot_vtx: the first caller vertex of every slot's triangle
// (device; null for a scene without triangles).  The instance is chosen by sc.n_sdfs
void launch_cast(const DevScene& sc, bool any_hit, const void* rays, uint32_t n, const uint32_t* slot_vtx, void* out, hipStream_t stream);
// prt_cast_pixels: the rays of the n pixels xy (device, n (x, y) pairs) of a width x full_height frame into rays (n prt_ray records)
void launch_cast_pixel_rays(const DevCamera& cam, int width, int full_height, const int32_t* xy, uint32_t n, void* rays, hipStream_t stream);

}  // namespace prt
