/*
 * ancsh_hip.h -- C ABI of libancsh_hip.so, the MI355X (gfx950) implementation of the ANCSH
 * inference + pose-fit hot path of dragonlong/articulated-pose.
 *
 * Drop-in boundary: these are the entry points a binding of the reference's native launchers
 * would call.  Each declaration cites the reference interface it replaces (paths relative to the
 * reference checkout; ops/ = pointnet_plusplus/utils/tf_ops/).  Conventions shared by all:
 *   - plain C: pointers + sizes only, no torch / TensorFlow types;
 *   - every buffer (inputs, outputs, scratch) is a caller-owned DEVICE pointer, row-major,
 *     float32 / int32; the library allocates nothing and keeps no mutable global state
 *     except a per-thread error string;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); launches are
 *     asynchronous, no hidden synchronisation;
 *   - return 0 on success, ANCSH_EINVAL (-1) on a bad argument (nothing launched),
 *     ANCSH_EHIP (-2) when HIP reports a launch error; ancsh_last_error() describes it.
 *     (The reference launchers return void and never check CUDA errors.)
 *
 * THROUGHPUT NOTE for a host that links this library directly.  The network kernels are throughput-bound, the pose fit is
 * latency-bound (stage B: one of a batch's 12 800 LM fits may run MINPACK's whole 4200-evaluation budget in a single lane, ~1.6 ms,
 * exactly as scipy does): a lone batch of 32 clouds takes ~3.5 ms, while >= 16 batches in flight on SEPARATE HIP streams sustain
 * ~1.57 ms per batch (bench.py keeps 20).  Streams share the process's hardware queues (GPU_MAX_HW_QUEUES, a host setting that
 * neither this library nor the Python package changes): where batches in flight outnumber the queues, one batch's LM kernel holds
 * back other batches' kernels queued behind it.  Create those streams ONCE and reuse them: a process that has used more than
 * ~20-24 distinct streams over its lifetime runs the same pipeline 5-25 % slower (every stream that has been used keeps a
 * hardware queue; profiles/r04_step_sensitivity.txt).  Nothing in this ABI creates streams or threads.
 */
#ifndef ANCSH_HIP_H
#define ANCSH_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define ANCSH_OK 0
#define ANCSH_EINVAL (-1)
#define ANCSH_EHIP (-2)

#define ANCSH_ACT_NONE 0
#define ANCSH_ACT_RELU 1
#define ANCSH_MAX_GROUPS 4 /* layers one grouped launch can hold (ancsh_*_grouped) */
#define ANCSH_ACT_RAW 2   /* y = the raw k-ordered accumulator: no bias, no BN (bias/scale/shift may be NULL) */

/* library / diagnostics */
int ancsh_abi_version(void);   /* added since without a new number (callers detect them by their symbols): ancsh_depth_unproject_stream,
                                 *     ancsh_depth_label_images (the depth front end and its label / NOCS images), ancsh_joint_state_rec (the
                                 *     streamed joint states), ancsh_fit_quality_rec (the streamed fit quality), ancsh_gt_error_rec (the streamed errors
                                 *     against ground truth), ancsh_point_gt_rec (the streamed per-point ground truth: test losses and joint errors), ancsh_point_gt_build (that ground truth built from
                                 *     annotated clouds), ancsh_depth_annotate_stream (those clouds made from depth and link-label crops),
                                 *     ancsh_render_depth_labels (those crops rendered from articulated triangle meshes),
                                 *     ancsh_pose_scene_build (that renderer's and the annotation's tables built from joint values and a view),
                                 *     ancsh_render_centre_crops (crops centred on the projected object),
                                 *     ancsh_depth_sensor_model, ancsh_depth_sensor_model_keyed (a depth sensor's noise, holes and edge dropout on those crops),
                                 *     ancsh_reproject_scene_build, ancsh_reproject_compare_rec (render-and-compare of a pose record),
                                 *     ancsh_refine_pass, ancsh_refine_rec (render-and-compare ICP: that record's poses refined on the depth frame),
                                 *     ancsh_silhouette_field, ancsh_refine_pass_sil (that loop's silhouette term: poses shifted across the ray come back),
                                 *     ancsh_coverage_field, ancsh_refine_pass_cov (its coverage term: a part is pulled over observed pixels it leaves bare),
                                 *     ancsh_refine_pass_scale (its scale unknown: with both pixel terms on, s is solved with R and t),
                                 *     ancsh_joint_values_rec (the streamed joint values: q read off the fitted and refined part poses),
                                 *ancsh_pose_fit_rec, ancsh_pose_fit_rec_dseed, ancsh_pose_fit_rec_dkey and their _kind forms (both
                                 *     stages of the pose fit in one call, the LM fits and stage A's refit in one launch);
                                 * 14: + ancsh_ransac_joint_rec_kind, ancsh_ransac_joint_rec_dseed_kind, ancsh_ransac_joint_rec_dkey_kind (a joint kind per
                                 *     stage-B problem: the prismatic objective);
                                 * 13: + ancsh_pose_joint_direction_pred, ancsh_pose_poison_records_pred, ancsh_input_sample_stream_xyz,
                                 *     ancsh_input_sample_stream_xyz_keyed (the joint association from the network's index head; xyz-only raw rows);
                                 * 12: + ancsh_raw_point_labels (per-raw-point labels and head values of a streamed batch);
                                 * 11: + ancsh_articulation_rec (the streamed articulation block);
                                 * 10: + ancsh_input_sample_stream_keyed, ancsh_ransac_single_rec_dkey, ancsh_ransac_joint_rec_dkey (ancsh_stream_key);
                                 * 9: + the F16x2 range guard (ancsh_*_f16x2*_guarded);
                                 * 8: + ancsh_input_sample_stream, ancsh_ransac_single_rec_dseed, ancsh_ransac_joint_rec_dseed (the streaming pipeline);
                                 * 7 since round 6 (5: round 5, 4: round 4, 3: round 3).  Operator entry points are only ever added: a library of version v serves every caller
                                 * written for <= v.  The one removal, in 7: ancsh_hbm_copy -- bench.py's HBM-copy yardstick, never an operator -- left the library
                                 * (tools/microbench/membw.hip, its own .so) */
const char *ancsh_last_error(void);

/* ---- PointNet++ set-abstraction / feature-propagation operators -------------------------- */

/* Replaces farthestpointsamplingLauncher(b,n,m,inp,temp,out), ops/sampling/tf_sampling_g.cu:203
 * (op shell ops/sampling/tf_sampling.cpp:95-123).  inp (b,n,3) -> out (b,m) int32; seed index 0;
 * ties resolved as the reference's 512-thread block does (lowest k%512, then lowest k).
 * `temp` is the reference's scratch argument (32*n floats there).  For n <= 8192 it may be NULL: coordinates and
 * running minimum distances live in registers.  n > 8192 takes the large-cloud kernel, which keeps the running
 * minima in `temp` and then REQUIRES it non-NULL with room for b*n floats (EINVAL otherwise). */
int ancsh_farthest_point_sample(int b, int n, int m, const float *inp, float *temp, int *out, void *stream);

/* Fused variant: also writes new_xyz (b,m,3) = gather_point(inp, out) (pointnet_util.py:47); `temp` as above. */
int ancsh_farthest_point_sample_gather(int b, int n, int m, const float *inp, float *temp, int *out_idx, float *out_xyz,
                                       void *stream);

/* Replaces probsampleLauncher(b,n,m,inp_p,inp_r,temp,out), ops/sampling/tf_sampling_g.cu:196 (op shell tf_sampling.cpp:66-92):
 * inp_p (b,n) non-negative weights, inp_r (b,m) uniform randoms in [0,1) -> out (b,m) int32 sampled indices by inverse CDF;
 * temp (b,n) float32 scratch receives the cumulative sums (same summation tree as the reference's block scan). */
int ancsh_prob_sample(int b, int n, int m, const float *inp_p, const float *inp_r, float *temp, int *out, void *stream);

/* Replaces gatherpointLauncher(b,n,m,inp,idx,out), ops/sampling/tf_sampling_g.cu:206. */
int ancsh_gather_point(int b, int n, int m, const float *inp, const int *idx, float *out, void *stream);

/* Replaces queryBallPointLauncher(b,n,m,radius,nsample,xyz1,xyz2,idx,pts_cnt),
 * ops/grouping/tf_grouping_g.cu:125.  xyz1 (b,n,3) dataset, xyz2 (b,m,3) queries ->
 * idx (b,m,nsample), pts_cnt (b,m).  A query with an empty ball gets idx = 0 and pts_cnt = 0
 * (the reference leaves those idx slots uninitialised). */
int ancsh_query_ball_point(int b, int n, int m, float radius, int nsample, const float *xyz1, const float *xyz2,
                           int *idx, int *pts_cnt, void *stream);

/* Up to four independent ball queries in ONE launch (arrays of length nprob): e.g. both set-abstraction levels of a batch --
 * level 2 only needs the level-1 centroids (ops/grouping/tf_grouping_g.cu:125 twice, pointnet_util.py:48 for layer1 and
 * layer2).  Outputs identical to nprob ancsh_query_ball_point calls. */
int ancsh_query_ball_point_multi(int nprob, const int *b, const int *n, const int *m, const float *radius, const int *nsample,
                                 const float *const *xyz1, const float *const *xyz2, int *const *idx, int *const *pts_cnt,
                                 void *stream);

/* query_ball_point + group_point(xyz1, idx) in one launch -- the first two ops of sample_and_group (pointnet_util.py:47-49):
 * idx / pts_cnt as above, grouped_xyz (b, m, nsample, out_ld >= 3) receives xyz1[idx] in its first three columns, minus the
 * query point when center != 0 (:49 `grouped_xyz -= new_xyz`).  Same results as the two separate ops. */
int ancsh_query_ball_group_xyz(int b, int n, int m, float radius, int nsample, const float *xyz1, const float *xyz2, int center,
                               int *idx, int *pts_cnt, float *grouped_xyz, int out_ld, void *stream);
/* The same for nprob <= 4 independent problems in ONE launch (arrays of length nprob; e.g. both set-abstraction levels of a batch).
 * Outputs identical to nprob ancsh_query_ball_group_xyz calls. */
int ancsh_query_ball_group_xyz_multi(int nprob, const int *b, const int *n, const int *m, const float *radius, const int *nsample,
                                     const float *const *xyz1, const float *const *xyz2, const int *center, int *const *idx,
                                     int *const *pts_cnt, float *const *grouped_xyz, const int *out_ld, void *stream);

/* Replaces groupPointLauncher(b,n,c,m,nsample,points,idx,out), ops/grouping/tf_grouping_g.cu:133.
 * b <= 65535 clouds per call (the cloud is a grid dimension); the same limit holds for the _ex form. */
int ancsh_group_point(int b, int n, int c, int m, int nsample, const float *points, const int *idx, float *out,
                      void *stream);

/* Up to four independent group_point problems (arrays of length nprob) in ONE launch: the grouped xyz of several SA levels
 * (pointnet_util.py:49 for layer1 and layer2) AND feature gathers with 16-byte rows (c % 4 == 0, 16-byte aligned buffers:
 * pointnet_util.py:51); a problem of any other channel count is launched on its own.  Outputs identical to nprob ancsh_group_point
 * calls. */
int ancsh_group_point_multi(int nprob, const int *b, const int *n, const int *c, const int *m, const int *nsample,
                            const float *const *points, const int *const *idx, float *const *out, void *stream);

/* Replaces selectionSortLauncher(b,n,m,k,dist,outi,out), ops/grouping/tf_grouping_g.cu:129 (select_top_k, tf_grouping.py:22):
 * dist (b,m,n) -> outi (b,m,n) int32, out (b,m,n): per row the k smallest in ascending order in the first k columns (ties: lowest
 * index first) and the remaining entries in the order the reference's swaps leave them.  n <= 7680. */
int ancsh_selection_sort(int b, int n, int m, int k, const float *dist, int *outi, float *out, void *stream);

/* knn_point(k, xyz1, xyz2), tf_grouping.py:48-74, in one launch: xyz1 (b,n,c) dataset, xyz2 (b,m,c) queries -> val (b,m,k) squared
 * distances ascending, idx (b,m,k) int32 = the first k columns of select_top_k over the pairwise squared distances. */
int ancsh_knn_point(int b, int n, int m, int c, int k, const float *xyz1, const float *xyz2, float *val, int *idx, void *stream);

/* group_point writing into a wider row: out[b,j,s, out_off : out_off+c] with row stride out_ld
 * floats; if center != NULL (b,m,c) it is subtracted (grouped_xyz -= new_xyz,
 * pointnet_util.py:53) -- fuses group + translation-normalisation + concat (:57). */
int ancsh_group_point_ex(int b, int n, int c, int m, int nsample, const float *points, const int *idx,
                         const float *center, float *out, int out_ld, int out_off, void *stream);

/* Replaces threenn_cpu(b,n,m,xyz1,xyz2,dist,idx), ops/3d_interpolation/tf_interpolate.cpp:60
 * (a host function in the reference).  dist = squared distances; m < 3 leaves +inf / index 0. */
int ancsh_three_nn(int b, int n, int m, const float *xyz1, const float *xyz2, float *dist, int *idx, void *stream);

/* pointnet_util.py:219-222: weight = (1/max(dist,1e-10)) / sum_3(1/max(dist,1e-10)); rows = b*n. */
int ancsh_three_weights(int rows, const float *dist, float *weight, void *stream);

/* ancsh_three_nn + ancsh_three_weights in one launch (same values). */
int ancsh_three_nn_weights(int b, int n, int m, const float *xyz1, const float *xyz2, float *dist, int *idx, float *weight,
                           void *stream);

/* Replaces threeinterpolate_cpu(b,m,c,n,points,idx,weight,out), tf_interpolate.cpp:107. */
int ancsh_three_interpolate(int b, int m, int c, int n, const float *points, const int *idx, const float *weight,
                            float *out, void *stream);

/* three_interpolate writing into out[b,j, out_off : out_off+c] with row stride out_ld (fuses the
 * concat of pointnet_util.py:226). */
int ancsh_three_interpolate_ex(int b, int m, int c, int n, const float *points, const int *idx,
                               const float *weight, float *out, int out_ld, int out_off, void *stream);

/* The input row of pointnet_fp_module in one launch (pointnet_util.py:218-229: three_interpolate, then
 * tf.concat([interpolated_points, points1])): out (b, n, out_ld) = [interpolated points2 (c2) | points1 (b, n, c1) | zeros].
 * Needs c2 % 4 == 0, out_ld % 4 == 0 >= c2 + c1, 16-byte aligned points2 / out; same arithmetic as ancsh_three_interpolate. */
int ancsh_fp_interpolate_concat(int b, int m, int c2, int n, const float *points2, const int *idx, const float *weight,
                                const float *points1, int c1, float *out, int out_ld, void *stream);

/* The same for several networks on the same clouds in one launch: points2 / out hold b clouds (network-major: the networks'
 * copies of cloud c are c, c + geo_batch, ...), the 3-NN arrays idx / weight hold geo_batch clouds and points1 holds
 * points1_batch (= b when every network has its own skip features, = geo_batch when the skip features are the input cloud
 * itself: fa_layer3, pointnet_plusplus/architectures.py:84); b % geo_batch == b % points1_batch == 0. */
int ancsh_fp_interpolate_concat_ex(int b, int m, int c2, int n, const float *points2, const int *idx, const float *weight,
                                   const float *points1, int c1, float *out, int out_ld, int geo_batch, int points1_batch,
                                   void *stream);

/* ---- shared per-point MLP (1x1 conv + bias + inference batch-norm + activation) ---------- */

/* Replaces tf_util.conv1d / conv2d with kernel 1x1 (+ batch_norm_for_conv*d + ReLU) as used by
 * pointnet_sa_module / pointnet_fp_module / the heads: pointnet_plusplus/utils/tf_util.py:52-185,
 * 512-531.  x (rows, cin) with row stride ldx; w (cin, cout) row-major (TF kernel [1,1,cin,cout]);
 * y = act( fma(acc + bias, scale, shift) ), acc = k-ordered f32 FMA chain (v_mfma_f32_32x32x2_f32);
 * scale/shift = folded inference BN (scale = gamma*rsqrt(var+1e-3), shift = beta - mean*scale;
 * pass ones/zeros for no BN).  y (rows, cout) with row stride ldy.
 * pool > 0: fuses tf.reduce_max over each run of `pool` consecutive rows (pointnet_util.py:134);
 * pool must be 64 or 128, rows % pool == 0, y is (rows/pool, cout). */
int ancsh_conv1x1(long rows, int cin, int cout, const float *x, int ldx, const float *w, const float *bias,
                  const float *scale, const float *shift, int act, float *y, int ldy, int pool, void *stream);

/* ancsh_conv1x1 whose accumulators do not start from zero: element (row, col) starts its k-ordered chain from
 * acc_init[row / init_rows][col] (acc_init: (ceil(rows/init_rows), cout) row-major, or NULL = plain ancsh_conv1x1).
 * With act = ANCSH_ACT_RAW on a first call over the leading input channels and acc_init on a second call over the
 * rest, the result is bit-identical to ONE call over the concatenated channels; pointnet_fp_module uses it when its
 * interpolation source is a single point per cloud (pointnet_util.py:218-229: the interpolated block is then the same
 * vector for every point, so its share of the dot product is computed once per cloud). */
int ancsh_conv1x1_ex(long rows, int cin, int cout, const float *x, int ldx, const float *w, const float *bias,
                     const float *scale, const float *shift, int act, float *y, int ldy, int pool, const float *acc_init,
                     int init_rows, void *stream);

/* ancsh_conv1x1_ex for wide layers (cout % 64 == 0) with the kernel in ancsh_sa_pack_weights' fragment order
 * (w_packed = ancsh_sa_pack_weights(cin, cout, w)).  Same results, bit for bit.  Two schedules: layers with 128 / 256 / 259 / 384
 * input channels, cout % 128 == 0 and no pooling take the small-layer schedule (csrc/conv_rowtile.hip: whole 32-row input tile in
 * LDS, any alignment of x); everything else the wave-independent kernel (csrc/conv_packed.hip: no barrier in the k loop), for
 * which x must be 16-byte aligned with ldx % 4 == 0. */
int ancsh_conv1x1_packed(long rows, int cin, int cout, const float *x, int ldx, const float *w_packed, const float *bias,
                         const float *scale, const float *shift, int act, float *y, int ldy, int pool,
                         const float *acc_init, int init_rows, void *stream);

/* GROUPED layer launches: the ANCSH and the NPCS network (main.py --nocs_type=ancsh / npcs) share their backbone's SHAPES
 * (pointnet_plusplus/architectures.py:62-86) and see the same clouds, so the same layer of both is evaluated in ONE launch on
 * stacked activations: group g (g < ngroups <= ANCSH_MAX_GROUPS) works on rows [g * rows, (g + 1) * rows) of x / y with its own
 * parameters w[g], bias[g], scale[g], shift[g] (host arrays of device pointers; bias / scale / shift may be NULL tables with
 * ANCSH_ACT_RAW).  `rows` is PER GROUP; acc_init holds ngroups * (rows / init_rows) rows (rows % init_rows == 0).  Every output
 * is the one the plain call computes, bit for bit.  The small layers these serve are latency-bound, so a second network's rows
 * ride along almost for free (4096 x 256 -> 256: 8.2 us alone, 12.7 us for two).
 * ancsh_conv1x1_packed_grouped: ancsh_conv1x1_packed per group.
 * ancsh_conv1x1_grouped: ancsh_conv1x1 per group (plain [cin][cout] kernels); one launch for the few-rows raw product
 * (rows <= 64 per group, ANCSH_ACT_RAW, no pooling), group by group otherwise. */
int ancsh_conv1x1_packed_grouped(int ngroups, long rows, int cin, int cout, const float *x, int ldx,
                                 const float *const *w_packed, const float *const *bias, const float *const *scale,
                                 const float *const *shift, int act, float *y, int ldy, int pool, const float *acc_init,
                                 int init_rows, void *stream);
int ancsh_conv1x1_grouped(int ngroups, long rows, int cin, int cout, const float *x, int ldx, const float *const *w,
                          const float *const *bias, const float *const *scale, const float *const *shift, int act, float *y,
                          int ldy, int pool, void *stream);

/* Whole body of pointnet_sa_module after sampling (pointnet_util.py:47-57 grouping + concat, :113-134 three shared-MLP
 * layers + max over nsample) in ONE launch; the grouped tensor and the per-layer activations stay in LDS.
 * xyz (b,n,3); new_xyz (b,m,3) and idx (b,m,64) from ancsh_farthest_point_sample_gather / ancsh_query_ball_point;
 * params = 12 device pointers {packed w, bias, scale, shift} for the 3 layers, where "packed w" is the layer's (cin_i, c_i)
 * kernel re-ordered ONCE by ancsh_sa_pack_weights; out (b*m, c3); nsample must be 64.  Results are bit-identical to the
 * unfused kernels (ancsh_group_point_ex + ancsh_conv1x1), which serve every other shape.
 *
 * ancsh_sa_module_fused: a level WITHOUT input features (cfeat must be 0, feats NULL): the ANCSH backbone's layer1, mlp 64,64,128
 * (pointnet_plusplus/architectures.py:62-65).
 *
 * ancsh_sa_module_fused_partial: a level WITH input features: layer2, mlp 128,128,256 (:66-70).  Its first layer's input row is
 * [x_j - c | f_j] (pointnet_util.py:55); the dot product is summed FEATURES FIRST, the three centred coordinates last (TensorFlow
 * does not define a summation order; every path of this library and the CPU oracle use this one).  The feature part does not
 * depend on the centroid, so the caller computes it once per SOURCE POINT --
 *     ancsh_conv1x1(b*n, c, c1, feats, c, w1 + 3*c1, NULL, NULL, NULL, ANCSH_ACT_RAW, partial, c1, 0, stream)
 * (kernel rows 3.. of the first layer) -- and passes `partial` (b,n,c1), 16-byte aligned; params[0] is then the packed kernel
 * rows 0..2 only (ancsh_sa_pack_weights(3, c1, w1, ...)).  The kernel gathers partial rows like feature rows and continues each
 * k-ordered chain with the coordinates: the layer costs n rows of matrix work instead of 64 m.
 *
 * SHAPE LIMITS (hard-coded kernel instantiations; anything else returns ANCSH_EINVAL before a launch and the caller --
 * pointnet_util.pointnet_sa_module -- takes the unfused ancsh_group_point_ex + ancsh_conv1x1 path with identical results):
 *   ancsh_sa_module_fused          cfeat == 0, (c1, c2, c3) == (64, 64, 128),   nsample == 64
 *   ancsh_sa_module_fused_partial  (c1, c2, c3) == (128, 128, 256),             nsample == 64
 * b * m <= 2^31 / 64 rows; any b, n, m otherwise. */
int ancsh_sa_module_fused(int b, int n, int m, int nsample, int cfeat, int c1, int c2, int c3, const float *xyz,
                          const float *feats, const float *new_xyz, const int *idx, const float *const *params, float *out,
                          void *stream);
int ancsh_sa_module_fused_partial(int b, int n, int m, int nsample, int c1, int c2, int c3, const float *xyz,
                                  const float *partial, const float *new_xyz, const int *idx, const float *const *params,
                                  float *out, void *stream);

/* The same level of `ngroups` networks on the SAME clouds in one launch (see ancsh_conv1x1_packed_grouped): the geometry (xyz,
 * new_xyz, idx) of b clouds is shared, feats / partial / out hold ngroups * b clouds network-major, params holds 12 pointers per
 * network.  Outputs identical to ngroups separate calls. */
int ancsh_sa_module_fused_grouped(int ngroups, int b, int n, int m, int nsample, int cfeat, int c1, int c2, int c3,
                                  const float *xyz, const float *feats, const float *new_xyz, const int *idx,
                                  const float *const *params, float *out, void *stream);
int ancsh_sa_module_fused_partial_grouped(int ngroups, int b, int n, int m, int nsample, int c1, int c2, int c3,
                                          const float *xyz, const float *partial, const float *new_xyz, const int *idx,
                                          const float *const *params, float *out, void *stream);

/* EXPERIMENT, opt-in (never the default path; f32 is the arithmetic of record): the same fused level with every f32 product
 * emulated on the bf16 matrix pipe -- activations and weights split exactly into three bf16 terms, six
 * v_mfma_f32_32x32x16_bf16 products per f32 product (csrc/sa_bf16x3.hip).  Each product is reproduced to f32 precision; the ORDER
 * of the additions inside the instruction differs from the k-ordered chain of ancsh_sa_module_fused, so results agree to f32
 * summation noise, not bit for bit.  Shape: cfeat == 0 (feats ignored), mlp (64,64,128), nsample 64.  params = {packed, bias,
 * scale, shift} x 3, all 16-byte aligned, with `packed` from ancsh_sa_pack_weights_bf16x3 (ancsh_sa_packed_weight_bytes_bf16x3(k, n)
 * bytes; n % 32 == 0). */
long ancsh_sa_packed_weight_bytes_bf16x3(int k, int n);
int ancsh_sa_pack_weights_bf16x3(int k, int n, const float *w, void *packed, void *stream);
int ancsh_sa_module_fused_bf16x3(int b, int n, int m, int nsample, int cfeat, int c1, int c2, int c3, const float *xyz,
                                 const float *feats, const float *new_xyz, const int *idx, const float *const *params, float *out,
                                 void *stream);
/* ... and the counterpart of ancsh_sa_module_fused_partial (mlp 128,128,256): `partial` = the first layer's raw f32 partial sums per
 * source point (as there), params[0] = ancsh_sa_pack_weights_bf16x3(3, c1, kernel rows 0..2); the whole MLP of a neighbourhood
 * stays in one wave's registers (hidden layers computed transposed, fragments re-formed with v_permlane32_swap), no LDS. */
int ancsh_sa_module_fused_partial_bf16x3(int b, int n, int m, int nsample, int c1, int c2, int c3, const float *xyz,
                                         const float *partial, const float *new_xyz, const int *idx, const float *const *params,
                                         float *out, void *stream);
/* ... and both for `ngroups` networks on the SAME clouds in one launch (the counterparts of ancsh_sa_module_fused_grouped /
 * ancsh_sa_module_fused_partial_grouped: shared geometry, partial / out network-major, 12 parameter pointers per network). */
int ancsh_sa_module_fused_bf16x3_grouped(int ngroups, int b, int n, int m, int nsample, int cfeat, int c1, int c2, int c3,
                                         const float *xyz, const float *feats, const float *new_xyz, const int *idx,
                                         const float *const *params, float *out, void *stream);
int ancsh_sa_module_fused_partial_bf16x3_grouped(int ngroups, int b, int n, int m, int nsample, int c1, int c2, int c3,
                                                 const float *xyz, const float *partial, const float *new_xyz, const int *idx,
                                                 const float *const *params, float *out, void *stream);
/* The same experiment with the F16x2 split scheme (csrc/bx3.h): x = hi + 2^-11 mid in two f16 terms, THREE v_mfma_f32_32x32x16_f16 products
 * into two accumulators instead of six bf16 products into one -- about 22 significant bits per operand (each product to ~7e-7 relative
 * instead of 6e-8), f16's range (|value| > 65504 -> inf -> the cloud's outputs NaN), half the matrix work.  Same arguments as the _bf16x3
 * entry points; weights packed by ancsh_sa_pack_weights_f16x2 (ancsh_sa_packed_weight_bytes_f16x2 bytes). */
long ancsh_sa_packed_weight_bytes_f16x2(int k, int n);
int ancsh_sa_pack_weights_f16x2(int k, int n, const float *w, void *packed, void *stream);
int ancsh_sa_module_fused_f16x2_grouped(int ngroups, int b, int n, int m, int nsample, int cfeat, int c1, int c2, int c3,
                                        const float *xyz, const float *feats, const float *new_xyz, const int *idx,
                                        const float *const *params, float *out, void *stream);
int ancsh_sa_module_fused_partial_f16x2_grouped(int ngroups, int b, int n, int m, int nsample, int c1, int c2, int c3,
                                                const float *xyz, const float *partial, const float *new_xyz, const int *idx,
                                                const float *const *params, float *out, void *stream);
/* RANGE GUARD of the F16x2 scheme: the six ancsh_*_f16x2*_guarded entry points take the arguments of their unguarded forms plus
 * range_flags / flag_bit0 and compute the same outputs, bit for bit.  range_flags holds one word per GEOMETRY cloud (b words); group g of
 * the launch ORs bit flag_bit0 + g into the word of every cloud for which some activation the scheme converts to f16 has |x| > 65504
 * (+-inf included; NaN never flags).  A paired launch (group 0 = ANCSH, 1 = NPCS) and two one-network launches with flag_bit0 = 0 / 1 fill
 * the same layout.  The words are only ever ORed: the caller zeroes them.  Weights are NOT checked (static: check them once on the host),
 * and neither is precision lost to f16's subnormal range (|x| < 2^-14).  Cost: one v_max3_f32 per converted value pair, one ballot per wave
 * and one atomic per flagged (wave, cloud).  Returns -1 before any launch for a NULL range_flags or flag_bit0 < 0 or flag_bit0 + ngroups > 32. */
int ancsh_sa_module_fused_f16x2_grouped_guarded(int ngroups, int b, int n, int m, int nsample, int cfeat, int c1, int c2, int c3,
                                                const float *xyz, const float *feats, const float *new_xyz, const int *idx,
                                                const float *const *params, float *out, unsigned *range_flags, int flag_bit0, void *stream);
int ancsh_sa_module_fused_partial_f16x2_grouped_guarded(int ngroups, int b, int n, int m, int nsample, int c1, int c2, int c3,
                                                        const float *xyz, const float *partial, const float *new_xyz, const int *idx,
                                                        const float *const *params, float *out, unsigned *range_flags, int flag_bit0,
                                                        void *stream);

/* Weight layout of ancsh_sa_module_fused: the MFMA B fragments of four consecutive k-steps as one 16-byte load per lane,
 *   packed[((slot*ceil(n/32) + j)*64 + lane)*4 + q] = w[2*(4*slot + q) + (lane >> 5)][j*32 + (lane & 31)]   (0 past row k-1 / column n-1).
 * ancsh_sa_packed_weight_floats(k, n) = number of floats `packed` must hold (-1 when k or n is not positive);
 * ancsh_sa_pack_weights re-orders a (k, n) row-major kernel on the device.  Done once per checkpoint, like the BN fold. */
long ancsh_sa_packed_weight_floats(int k, int n);
int ancsh_sa_pack_weights(int k, int n, const float *w, float *packed, void *stream);

/* A chain of per-point shared-MLP layers in ONE launch (the tail of the ANCSH graph: fa_layer3 convs, fc1, the
 * NOCS heads and the joint heads -- pointnet_plusplus/architectures.py:84-93, lib/architecture.py:105-129,195-206);
 * activations stay in two LDS tiles, only head logits are written.  x (rows, cin <= 131) with row stride ldx is
 * loaded into tile 0; op i computes act(BN(tile[src] . w + b)) with w (k, n), n == 128 or n <= 32, into tile dst
 * (0 or 1; dst == src runs the layer in place) or, when dst == -1, into the global matrix out (rows, n) with row stride out_ld.
 * ops: nops x 6 ints {k, n, act, src, dst, out_ld}; ptrs: nops x 5 device pointers {packed w, bias, scale, shift, out|NULL},
 * packed w = ancsh_sa_pack_weights(k, n, w) (any n: columns are zero-padded to a multiple of 32).
 * Each layer is the same arithmetic as ancsh_conv1x1 (bit-identical results). */
int ancsh_mlp_chain(long rows, int cin, const float *x, int ldx, int nops, const int *ops, const void *const *ptrs,
                    void *stream);

/* The same chain with ONE LDS tile per wave -- two waves per SIMD instead of one -- for ngroups <= 2 networks in one launch
 * (round 4).  Group g reads rows [g * rows, (g + 1) * rows) of x (row stride ldx) and runs ITS program.  Every 128-column layer
 * rewrites the wave's tile in place; a head block (n <= 32) writes (rows, n) to its global matrix `out` with row stride out_ld.
 * ops[g]: nops[g] x 5 ints {k, n, act, flags, out_ld}; ptrs[g]: nops[g] x 5 device pointers {packed w, bias, scale, shift, out | NULL}.
 * flags: 1 = the layer's 128-column output is also copied to this network's rows of `scratch`; 2 = the tile is reloaded from
 * them before the layer runs (the trunk `net` of lib/architecture.py:104 feeds both fc11_1 and fc3_0).  scratch: ngroups * rows * 128
 * floats, 16-byte aligned; NULL when no op carries a flag.  Bit-identical to ancsh_mlp_chain / ancsh_conv1x1. */
int ancsh_mlp_chain_grouped(int ngroups, long rows, int cin, const float *x, int ldx, const int *nops, const int *const *ops,
                            const void *const *const *ptrs, float *scratch, void *stream);

/* The MIDDLE of the backbone as chain launches (round 5, csrc/mid_chain.hip): layer3 (sample_and_group_all + 3 conv2d + reduce_max,
 * pointnet_util.py:66-91,113-134 via pointnet_plusplus/architectures.py:72-75), fa_layer1 and fa_layer2 (three_interpolate + concat +
 * 2 conv2d, pointnet_util.py:206-236 via architectures.py:78-82) of `ngroups` networks on the same b clouds.  A workgroup owns a 32-row
 * tile for a whole level, the layers' columns are split over its waves, activations never leave LDS; every output is bit-identical to
 * the layer-by-layer calls (ancsh_conv1x1_packed / ancsh_fp_interpolate_concat).  "packed w" = ancsh_sa_pack_weights of the layer's
 * (cin, cout) kernel.  Hard-coded instantiations -- the ANCSH backbone widths; any other shape returns ANCSH_EINVAL before a launch:
 *
 * ancsh_sa3_chain_grouped: xyz (b, npts, 3) shared by the networks, feats (ngroups * b, npts, cfeat = 256) network-major, npts % 32 == 0;
 *   params = per network 3 x {packed w, bias, scale, shift} for (3 + cfeat) -> c1 = 256 -> c2 = 512 -> c3 = 1024 (input row = [xyz | feats],
 *   pointnet_util.py:88); out (ngroups * b, npts / 32, c3): the maxima over each 32-row tile -- a cloud's output row is the element-wise
 *   maximum of its npts / 32 rows (taken by ancsh_fp_single_source_init; max is exact in any order).
 * ancsh_fp_single_source_init: the share of an FP module's first layer that comes from a ONE-point interpolation source
 *   (pointnet_util.py:218-224 with m == 1: weights exactly (1, 0, 0), so every point receives the source row): y (ngroups * b, cout) =
 *   the RAW k-ordered chain of max_q x[row][q][0:cin] over the plain kernel rows w[g][0:cin][0:cout]; x (ngroups * b, nparts, cin);
 *   cin % 64 == 0, cout % 128 == 0, x 16-byte aligned.
 * ancsh_fp1_chain_grouped: skip (ngroups * b * npts, cskip = 256), init (ngroups * b, c1) from the call above (row / npts selects it);
 *   params = per network 2 x {packed w, bias, scale, shift}: the first layer's kernel rows [cin_source:] (cskip -> c1 = 256) and the
 *   second layer (c1 -> c2 = 256); out (ngroups * b * npts, c2).
 * ancsh_fp2_chain_grouped: points2 (ngroups * b, m, c2 = 256) interpolation source, idx / weight (b, n, 3) of the shared geometry
 *   (ancsh_three_nn_weights), points1 (ngroups * b, n, c1 = 128) skip features, n % 32 == 0; the interpolation is
 *   p[i1] * w1 + p[i2] * w2 + p[i3] * w3 in that order (tf_interpolate.cpp:107-127); params = per network 2 x {packed w, bias, scale,
 *   shift} for (c2 + c1) -> n1 = 256 -> n2 = 128; out (ngroups * b * n, n2).
 * feats / skip / points2 / points1 and the packed kernels must be 16-byte aligned. */
int ancsh_sa3_chain_grouped(int ngroups, int b, int npts, int cfeat, int c1, int c2, int c3, const float *xyz, const float *feats,
                            const float *const *params, float *out, void *stream);
int ancsh_fp_single_source_init(int ngroups, int b, int cin, int cout, int nparts, const float *x, const float *const *w, float *y,
                                void *stream);
int ancsh_fp1_chain_grouped(int ngroups, int b, int npts, int cskip, int c1, int c2, const float *skip, const float *init,
                            const float *const *params, float *out, void *stream);
int ancsh_fp2_chain_grouped(int ngroups, int b, int m, int n, int c2, int c1, int n1, int n2, const float *points2, const int *idx,
                            const float *weight, const float *points1, const float *const *params, float *out, void *stream);

/* Diagnostic: the schedule the last ball-query launch of this process took (-1 wave per two queries = the default, 0..2 the opt-in
 * lane = query kernel selected with ANCSH_BQ_SCHEDULE=lanes<k>, -2 none yet).  A lanes<k> request that exceeds the kernel's LDS / word
 * limits falls back to the default schedule; results are identical either way (tests/test_ops_gpu.py). */
int ancsh_last_ball_query_schedule(void);

/* Round 5: ancsh_mlp_chain_grouped whose input rows are fa_layer3's [three_interpolate(points2) (c2 = 128) | xyz (3)]
 * (pointnet_util.py:218-229 via pointnet_plusplus/architectures.py:84-86) BUILT IN THE TILE LOAD: no (b * n, 132) concat buffer is written
 * or read and the interpolate + concat launch disappears.  points2 (ngroups * b, m, 128) network-major, 16-byte aligned; idx / weight
 * (b, n, 3) from ancsh_three_nn_weights and xyz (b, n, 3) are shared by the networks; n % 128 == 0; rows per network = b * n; nops / ops /
 * ptrs / scratch as ancsh_mlp_chain_grouped (the first op has k = 131).  Interpolation p[i1] * w1 + p[i2] * w2 + p[i3] * w3 in that order
 * (tf_interpolate.cpp:107-127): bit-identical to ancsh_fp_interpolate_concat_ex + ancsh_mlp_chain_grouped. */
int ancsh_mlp_chain_grouped_fp(int ngroups, int b, int n, int m, int c2, const float *points2, const int *idx, const float *weight,
                               const float *xyz, const int *nops, const int *const *ops, const void *const *const *ptrs, float *scratch,
                               void *stream);

/* EXPERIMENT, opt-in (like ancsh_sa_module_fused_bf16x3; f32 is the arithmetic of record): ancsh_mlp_chain_grouped_fp with every f32
 * product emulated by six bf16 MFMA products (csrc/tail_bf16x3.hip).  A wave owns 64 points and keeps their 128-channel activations in
 * registers as bf16x3 fragments (two register tiles: no save / restore of the trunk); n % 64 == 0.  ops[g]: nops[g] x 5 ints {k, n, act,
 * 0, out_ld}; ptrs[g]: nops[g] x 5 pointers {w packed by ancsh_sa_pack_weights_bf16x3, bias, scale, shift, out | NULL}, all 16-byte
 * aligned; a head block (out != NULL) is 128 -> n <= 32 with w packed as (128, 32) and bias / scale / shift holding 32 entries.  The op
 * list must have the shape  F H H H head+ [L head+] H H head+  (F = 131 -> 128 ReLU, H = 128 -> 128 ReLU, L = 128 -> 128 linear): the tail
 * of lib/architecture.py:98-139,195-208 with and without early_split_nocs. */
int ancsh_mlp_chain_grouped_fp_bf16x3(int ngroups, int b, int n, int m, int c2, const float *points2, const int *idx, const float *weight,
                                      const float *xyz, const int *nops, const int *const *ops, const void *const *const *ptrs,
                                      void *stream);
int ancsh_mlp_chain_grouped_fp_f16x2(int ngroups, int b, int n, int m, int c2, const float *points2, const int *idx, const float *weight,
                                     const float *xyz, const int *nops, const int *const *ops, const void *const *const *ptrs,
                                     void *stream);      /* the F16x2 scheme; weights packed by ancsh_sa_pack_weights_f16x2 */
int ancsh_mlp_chain_grouped_fp_f16x2_guarded(int ngroups, int b, int n, int m, int c2, const float *points2, const int *idx, const float *weight,
                                             const float *xyz, const int *nops, const int *const *ops, const void *const *const *ptrs,
                                             unsigned *range_flags, int flag_bit0, void *stream);     /* ... with the range guard (see above) */

/* ... and the MIDDLE of the backbone (ancsh_sa3_chain_grouped / ancsh_fp1_chain_grouped / ancsh_fp2_chain_grouped) on the 16-bit matrix pipe
 * (csrc/mid_bf16x3.hip): the activations of a 64-row tile live in LDS as the scheme's 16-bit planes, the workgroup's waves split every layer
 * by output channels.  Same arguments as the f32 forms with kernels packed by ancsh_sa_pack_weights_{bf16x3,f16x2} and 16-byte aligned bias /
 * scale / shift; npts (n) % 64 == 0, and layer3's out is (ngroups * b, npts / 64, 1024): the maxima of every 64-ROW tile (pass nparts =
 * npts / 64 to ancsh_fp_single_source_init).  ancsh_sa3_chain_grouped_bf16x3 returns an error: three bf16 planes of a 64 x 512 tile exceed the
 * 160 KB of LDS (layer3 then takes the f32 chain). */
int ancsh_sa3_chain_grouped_bf16x3(int ngroups, int b, int npts, int cfeat, int c1, int c2, int c3, const float *xyz, const float *feats,
                                   const float *const *params, float *out, void *stream);
int ancsh_sa3_chain_grouped_f16x2(int ngroups, int b, int npts, int cfeat, int c1, int c2, int c3, const float *xyz, const float *feats,
                                  const float *const *params, float *out, void *stream);
int ancsh_fp1_chain_grouped_bf16x3(int ngroups, int b, int npts, int cskip, int c1, int c2, const float *skip, const float *init,
                                   const float *const *params, float *out, void *stream);
int ancsh_fp1_chain_grouped_f16x2(int ngroups, int b, int npts, int cskip, int c1, int c2, const float *skip, const float *init,
                                  const float *const *params, float *out, void *stream);
int ancsh_fp2_chain_grouped_bf16x3(int ngroups, int b, int m, int n, int c2, int c1, int n1, int n2, const float *points2, const int *idx,
                                   const float *weight, const float *points1, const float *const *params, float *out, void *stream);
int ancsh_fp2_chain_grouped_f16x2(int ngroups, int b, int m, int n, int c2, int c1, int n1, int n2, const float *points2, const int *idx,
                                  const float *weight, const float *points1, const float *const *params, float *out, void *stream);
/* ... the F16x2 forms with the range guard (see ancsh_sa_module_fused_f16x2_grouped_guarded) */
int ancsh_sa3_chain_grouped_f16x2_guarded(int ngroups, int b, int npts, int cfeat, int c1, int c2, int c3, const float *xyz, const float *feats,
                                          const float *const *params, float *out, unsigned *range_flags, int flag_bit0, void *stream);
int ancsh_fp1_chain_grouped_f16x2_guarded(int ngroups, int b, int npts, int cskip, int c1, int c2, const float *skip, const float *init,
                                          const float *const *params, float *out, unsigned *range_flags, int flag_bit0, void *stream);
int ancsh_fp2_chain_grouped_f16x2_guarded(int ngroups, int b, int m, int n, int c2, int c1, int n1, int n2, const float *points2, const int *idx,
                                          const float *weight, const float *points1, const float *const *params, float *out,
                                          unsigned *range_flags, int flag_bit0, void *stream);

/* tf.reduce_max over nsample (pointnet_util.py:134): x (groups, nsample, c) -> y (groups, c). */
int ancsh_group_max(long groups, int nsample, int c, const float *x, float *y, void *stream);

/* ANCSH head activations + gocs composition, lib/architecture.py:124-159.
 *  logits (rows, ld) holds, per point, the raw head outputs laid out as
 *    [W(K) | nocs(3K) | scale(K) | trans(3K) | confi(1) | axis(3) | unitvec(3) | heatmap(1) | joint_cls(3)]
 *  (mixed_pred = 1, ANCSH) or [W(K) | nocs(3K) | confi(1) | axis(3) | unitvec(3) | heatmap(1) | joint_cls(3)]
 *  (mixed_pred = 0, NPCS).  Outputs (any may be NULL): W softmax (rows,K); nocs sigmoid (rows,3K);
 *  confi sigmoid (rows,1); heatmap sigmoid (rows,1); unitvec tanh (rows,3); axis tanh (rows,3);
 *  joint_cls softmax (rows,3); gocs = nocs*repeat(scale,3)+trans (rows,3K); scale sigmoid (rows,K);
 *  trans tanh (rows,3K). */
int ancsh_head_activations(long rows, int K, int mixed_pred, const float *logits, int ld, float *W, float *nocs,
                           float *confi, float *heatmap, float *unitvec, float *axis, float *joint_cls,
                           float *gocs, float *scale, float *trans, void *stream);

/* ---- pose fitting (host Python + numpy/scipy in the reference; device kernels here) ----------- */

/* Front end of the per-cloud loop body of solver_ransac_nonlinear (evaluation/parallel_ancsh_pose.py
 * :238-242, 259-260): labels = argmax(W, axis=1) (first maximum wins); the cloud's points are
 * partitioned by label in ascending point order, and the per-part (source, target) arrays
 *   source = nocs[idx, 3j:3j+3] (the point's own part-NOCS slot), target = P[idx, :3]
 * are written packed: rows [off[b*K+j], off[b*K+j+1]) of src/tgt (b*n rows in total, off has b*K+1
 * entries).  W (b,n,K), P (b,n,3), nocs (b,n,3K); labels (b,n) may be NULL; part_index (b,n) holds
 * the original point id of every packed row.  Optional by-products (NULL to skip): counts (b,K) points per part; rng0 / rng1
 * (b*(K-1), 2) = the [start,end) packed-row ranges of part 0 and of part j for every joint j = 1..K-1, i.e. the arguments
 * ancsh_ransac_joint takes (:274-283). */
int ancsh_pose_partition(int b, int n, int K, const float *W, const float *P, const float *nocs, int *labels,
                         int *part_index, int *off, float *src, float *tgt, int *counts, int *rng0, int *rng1, void *stream);

/* Non-finite inputs of the fit: a cloud whose P (b,n,3), nocs (b,n,3K), W (b,n,K) or joint_axis (b,n,3; may be NULL) holds a NaN or
 * +-Inf has no defined pose (in the reference np.linalg.svd raises LinAlgError on such a part, lib/d3_utils.py:214; np.argmax /
 * np.median over NaN rows are arbitrary): every value of its record (b, K, 26) float64 rows is set to NaN.  Call after the fit
 * kernels that write `record`; clouds without a non-finite value are not touched. */
int ancsh_pose_poison_records(int b, int n, int K, const float *P, const float *nocs, const float *W, const float *joint_axis,
                              double *record, void *stream);

/* ancsh_pose_poison_records for a fit whose joint association comes from the ANCSH network's index head (ABI 13): the same scan plus
 * joint_index (b, n, joint_channels) float32, so a non-finite value there poisons the cloud's record as well.  The predicted-association
 * fit calls this INSTEAD of ancsh_pose_poison_records (one launch either way).  Checked before any launch: the shape, 1 <= joint_channels
 * <= 64, null pointers (joint_axis may be NULL). */
int ancsh_pose_poison_records_pred(int b, int n, int K, const float *P, const float *nocs, const float *W, const float *joint_axis,
                                   int joint_channels, const float *joint_index, double *record, void *stream);

/* jt_axis = np.median(joint_axis_per_point[joint_cls == j], 0), j = 1..K-1 (:295).
 * joint_axis (b,n,3), joint_cls (b,n) int32 -> out (b, K-1, 3) float32 (NaN for an empty selection). */
int ancsh_pose_joint_direction(int b, int n, int K, const float *joint_axis, const int *joint_cls, float *out,
                               void *stream);

/* jt_axis = np.median(joint_axis_per_point[np.argmax(joint_index, 1) == j], 0), j = 1..K-1 (lib/parallel_ancsh_pose.py:339-343,366;
 * evaluation/eval_joint_params.py:133-134): the joint association taken from the ANCSH network's index head instead of a label array
 * (ABI 13).  joint_index (b, n, joint_channels) float32; the argmax is np.argmax's (the first maximum; a row holding a NaN selects its
 * first NaN channel), taken while compacting, in the same launch.  The result is the bytes of ancsh_pose_joint_direction fed
 * np.argmax(joint_index, -1).astype(np.int32) -- NaN for a joint no point selects.  Such a joint is CERTAIN when K - 1 >= joint_channels
 * (the reference's rule: drawer, K = 4, with the 3-wide head never selects joint 3).  Checked before any launch: 2 <= K <= 16,
 * 1 <= n <= 8192, 1 <= joint_channels <= 64, null pointers. */
int ancsh_pose_joint_direction_pred(int b, int n, int K, int joint_channels, const float *joint_axis, const float *joint_index,
                                    float *out, void *stream);

/* THE FIT ENTRIES AT A GLANCE.  Nineteen entries, one fit: each is the per-part fit (stage A, ancsh_ransac_single*), the per-joint fit
 * (stage B, ancsh_ransac_joint*) or both in one call (ancsh_pose_fit_rec*), with the generator key passed in one of three ways and,
 * for stage B, an optional joint kind per problem.  The blocks below state each rule once, where it first applies.
 *
 *   key mode    suffix   key argument                            stage A reads       stage B reads       problem index of the generator
 *   by value    (none)   unsigned long long seed                 seed                seed (the caller    prob
 *                                                                                    passes s + 1)
 *   device seed _dseed   const unsigned long long *seed          *seed               *seed + 1           prob
 *   key block   _dkey    const ancsh_stream_key *key (needs K)   key->seed           key->seed + 1       prob + key->cloud_base * K  (stage A)
 *                                                                                                        prob + key->cloud_base * (K - 1)  (B)
 *
 *   stage A: ancsh_ransac_single, _ex (+ scratch_quads, rows), _rec (+ record, K, tie_stats, tie_window), _rec_dseed, _rec_dkey
 *   stage B: ancsh_ransac_joint, _ex (+ lm_schedule), _rec (+ record, K, tie_stats, tie_window), _rec_dseed, _rec_dkey
 *   both:    ancsh_pose_fit_rec, _rec_dseed, _rec_dkey
 *   _kind behind any stage-B or whole-fit _rec name: one more argument, const int *joint_kind, before the stream (NULL = the entry
 *   without the suffix).
 * All of them are adapters over one host-side description of a fit call (csrc/pose.hip): the same argument checks in the same order,
 * the same launches. */

/* Batched replacement of ransac(dataset, single_transformation_estimator, single_transformation_verifier,
 * inlier_th, niter) (:20-54, with transform_pts / rotate_pts / scale_pts of lib/d3_utils.py:206-246).
 * Problem p = rows [off[p], off[p+1]) of src/tgt (float32 (rows,3)).  draws (nprob, niter, 3) int32 =
 * the 3-point sample of every iteration (the reference draws np.random.randint(n, size=3) from the global
 * RNG, :38); NULL -> on-device counter-based generator keyed by `seed`.  max_n >= every problem size.
 * out_model (nprob,13) float64: R row-major (9), scale, translation (3) of the full-inlier refit;
 * out_inliers (rows) uint8 mask of the winning hypothesis; out_best (nprob,2): winning iteration (ties ->
 * earliest) and its inlier count.  scratch_scores: nprob*niter int32.  An empty problem yields NaNs and
 * out_best = (-1, 0) (the reference raises). */
int ancsh_ransac_single(int nprob, const int *off, const float *src, const float *tgt, float inlier_th, int niter,
                        const int *draws, unsigned long long seed, int max_n, double *out_model,
                        unsigned char *out_inliers, int *out_best, int *scratch_scores, void *stream);

/* ancsh_ransac_single with the hypotheses scored from SCALAR registers.  Every lane of a wave tests the same point (lane =
 * hypothesis), so the points are wave-uniform operands: a padded copy of each part, four points per 96-byte record
 * {x[4] y[4] z[4]} source | {x[4] y[4] z[4]} target (scratch_quads, written by the call itself), is read with s_load_dwordx8/x16
 * and enters the packed-f32 residual arithmetic as the instruction's scalar source -- no LDS, no barrier, no staging pass per
 * workgroup.  scratch_quads: 32-byte aligned, ancsh_ransac_single_quads_floats(rows, nprob) floats where rows >= off[nprob]
 * (the row capacity of src/tgt; the kernels never write or read past that capacity even if off[] exceeds it).  Scores, winner,
 * inlier mask and model are those of ancsh_ransac_single bit for bit (evaluation/parallel_ancsh_pose.py:20-54, same replacement). */
long ancsh_ransac_single_quads_floats(long rows, int nprob);
int ancsh_ransac_single_ex(int nprob, const int *off, const float *src, const float *tgt, float inlier_th, int niter,
                           const int *draws, unsigned long long seed, int max_n, double *out_model,
                           unsigned char *out_inliers, int *out_best, int *scratch_scores, float *scratch_quads, long rows,
                           void *stream);

/* Round 5: ancsh_ransac_single_ex (scratch_quads != NULL) / ancsh_ransac_single (NULL) with two optional extra outputs; scores,
 * winner, mask and out_model bit for bit as before.
 *   record (B, K, 26) float64, B = nprob / K: the per-part pose record the reference assembles in Python
 *     (evaluation/parallel_ancsh_pose.py:330-353), row (b, j) = [baseline R(9) s t(3) | nonlinear R(9) s t(3)]: this call fills columns
 *     0..12 of row p (and 13..25 when K == 1), ancsh_ransac_joint_rec columns 13..25 -- no assembly launches (torch.cat / clone) in
 *     the captured step.  NULL: not written.
 *   tie_stats (nprob, 2) int32 -- how implementation-sensitive the fit is:
 *     [0] points of the part whose residual norm under the WINNING hypothesis lies in [inlier_th - tie_window, inlier_th + tie_window)
 *         -- the verifier's `sqrt(sum(res**2)) < th` (:48-54) is a float32 threshold test, and an implementation whose 3-point model
 *         differs in the last bits (LAPACK's SVD there, Horn's quaternion here) may count such a point on the other side;
 *     [1] DEGENERATE CONTENDERS THAT WOULD CHANGE THE CONSENSUS SET: hypotheses whose score is within one inlier of the winning score,
 *         whose 3-point sample repeats an index (np.random.randint draws WITH replacement, :38) and which -- had they won -- would have
 *         handed the refit another inlier mask than the winner's (the winner itself counts once when its own sample is degenerate; of
 *         the others the 16 lowest-numbered hypotheses are examined, and any beyond them are counted as changing: the count is the same
 *         from run to run and from launch to launch).  Until
 *         round 5 every degenerate contender was counted (20-25 % of the fits at N = 1024: nearly all of them hypotheses with the
 *         winner's own mask, which cannot change the result whoever scores them).  The count is NEGATIVE when the winner's own sample is
 *         degenerate, and only then (read from the winner's own sample: exact however many contenders there are) -- the one case in
 *         which the fit's consensus set is implementation-defined for certain (measured at 10000 / 200 on
 *         624 fits, profiles/r06_pose_tie_rate_K3.txt: 3 such fits, all 3 on another set than the reference arithmetic; a positive count
 *         fired on 22.9 % of the fits and held 1 of the other 4 flips: as a per-fit warning only the sign is sharp).  The centred points of such a sample are
 *         collinear, the 3 x 3 covariance has rank 1, and the rotation the reference takes from np.linalg.svd (lib/d3_utils.py:214) is
 *         LAPACK's completion of a null space that rounding noise selects -- implementation-defined in the reference itself.
 *     Measured at the reference's budgets on 1344 clouds, 8064 reported fits (profiles/r05_pose_tie_rate_full.txt): [0] was 0 in EVERY fit
 *     -- no threshold-tie flips at 10000 / 200 --; 32 fits (0.40 %) ended on another consensus set than the reference arithmetic, ALL
 *     with a repeated-index winner on one side; [1] > 0 in 22 of those 32 (and in 20-25 % / 5-10 % of all fits at N = 1024 / 2048) -- it
 *     sees the degenerate contenders of THIS implementation's arithmetic, while the other 10 had a degenerate winner only under LAPACK's
 *     choice of the free rotation about the sample's line, which no other implementation can score.
 *     NULL: not computed.  tie_window: absolute half-width on the norm, 0 <= tie_window < inlier_th. */
int ancsh_ransac_single_rec(int nprob, const int *off, const float *src, const float *tgt, float inlier_th, int niter,
                            const int *draws, unsigned long long seed, int max_n, double *out_model, unsigned char *out_inliers,
                            int *out_best, int *scratch_scores, float *scratch_quads, long rows, double *record, int K,
                            int *tie_stats, float tie_window, void *stream);

/* Batched replacement of ransac(dataset, joint_transformation_estimator, joint_transformation_verifier,
 * inlier_th, niter) (:20-33, 106-194; revolute objective :56-68; scipy least_squares(method='lm',
 * ftol=1e-4) = MINPACK lmdif restated on the 6x6 normal equations).  Problem p couples part 0
 * (rows [rng0[2p], rng0[2p+1])) and part j (rows [rng1[2p], rng1[2p+1])) of src/tgt through the joint
 * direction joint_dir[p] (3).  draws (nprob, niter, 6) int32 (3 samples of part 0, then 3 of part j) or
 * NULL.  out_model (nprob,26) float64: R0(9) s0 t0(3) R1(9) s1 t1(3) of the all-inlier refit;
 * out_inliers (nprob, 2, max_n) uint8; out_best (nprob) winning iteration; out_score (nprob) its score
 * ((n_inl0/3 + n_inl1/3)/2 as in :192).  scratch_scores nprob*niter float64, scratch_models
 * nprob*niter*26 float64, lm_stat (nprob,niter,2) int32 (MINPACK info, nfev) or NULL. */
int ancsh_ransac_joint(int nprob, const int *rng0, const int *rng1, const float *src, const float *tgt,
                       const float *joint_dir, double inlier_th, int niter, const int *draws,
                       unsigned long long seed, int max_n, double *out_model, unsigned char *out_inliers,
                       int *out_best, double *out_score, double *scratch_scores, double *scratch_models,
                       int *lm_stat, void *stream);

/* The same with an explicit schedule for the per-hypothesis LM fits.  Both schedules run the same MINPACK state machine; their
 * floating-point results agree to ~1e-7 (the eight-lane schedule recombines partial sums through a different instruction stream),
 * far inside the 1e-4 parity bar, and pick the same winning hypotheses on every test -- but NOT bit for bit.  The schedule is
 * therefore never chosen from the launch size: a cloud solved alone and the same cloud inside a batch of 32 give identical bytes
 * (tests/test_pose_gpu.py::test_stage_b_is_batch_size_invariant).
 *   ANCSH_LM_AUTO       = ANCSH_LM_THROUGHPUT (round 4; until round 3 launches of <= 2048 fits took the eight-lane schedule);
 *   ANCSH_LM_THROUGHPUT one lane per fit: least SIMD time; a small launch hands fewer hypotheses to each wave (scheduling only);
 *   ANCSH_LM_LATENCY    eight lanes per fit: the launch's long fits finish ~1.25x sooner, ~5 % less pipeline throughput.
 *                       Explicit only (AncshPipeline selects it for <= 2 batches in flight, a latency deployment). */
#define ANCSH_LM_AUTO 0
#define ANCSH_LM_THROUGHPUT 1
#define ANCSH_LM_LATENCY 2
int ancsh_ransac_joint_ex(int nprob, const int *rng0, const int *rng1, const float *src, const float *tgt,
                          const float *joint_dir, double inlier_th, int niter, const int *draws,
                          unsigned long long seed, int max_n, double *out_model, unsigned char *out_inliers,
                          int *out_best, double *out_score, double *scratch_scores, double *scratch_models,
                          int *lm_stat, int lm_schedule, void *stream);

/* ancsh_ransac_joint_ex with the same two optional outputs (see ancsh_ransac_single_rec): problem p = b * (K - 1) + q writes columns
 * 13..25 of record row (b, q + 1) and -- q == 0 -- of row (b, 0) (part 0 is reported from joint 1's fit, :327-329); tie_stats
 * (nprob, 2): [0] points of BOTH parts within tie_window of the threshold under the winning hypothesis' model (float64 test,
 * :186-194), [1] degenerate contenders: hypotheses within one inlier (1/6 of the joint score, :192) of the winning score with a
 * repeated index in either 3-point sample (:110-111). */
int ancsh_ransac_joint_rec(int nprob, const int *rng0, const int *rng1, const float *src, const float *tgt,
                           const float *joint_dir, double inlier_th, int niter, const int *draws, unsigned long long seed,
                           int max_n, double *out_model, unsigned char *out_inliers, int *out_best, double *out_score,
                           double *scratch_scores, double *scratch_models, int *lm_stat, int lm_schedule, double *record, int K,
                           int *tie_stats, double tie_window, void *stream);

/* ancsh_ransac_single_rec / ancsh_ransac_joint_rec with the generator key in DEVICE memory: `seed` points at one uint64 that the
 * kernels read when they run, so a captured graph replays with whatever the host last wrote there (a fresh sample stream per batch;
 * the by-value key is frozen into the graph).  Stage A uses *seed, stage B *seed + 1 -- the pair PoseSolver.solve(seed=s) passes to
 * the by-value entries (s, s + 1) -- so solve(seed_dev=[s]) gives the bytes of solve(seed=s).  Explicit draws still override the
 * generator.  The kernels are the by-value ones instantiated with the key read once per kernel; the by-value entries are unchanged
 * (same code, registers and occupancy: profiles/r07_pose_resource_usage_{before,after}.txt).  seed == NULL is refused. */
int ancsh_ransac_single_rec_dseed(int nprob, const int *off, const float *src, const float *tgt, float inlier_th, int niter,
                                  const int *draws, const unsigned long long *seed, int max_n, double *out_model,
                                  unsigned char *out_inliers, int *out_best, int *scratch_scores, float *scratch_quads, long rows,
                                  double *record, int K, int *tie_stats, float tie_window, void *stream);
int ancsh_ransac_joint_rec_dseed(int nprob, const int *rng0, const int *rng1, const float *src, const float *tgt,
                                 const float *joint_dir, double inlier_th, int niter, const int *draws, const unsigned long long *seed,
                                 int max_n, double *out_model, unsigned char *out_inliers, int *out_best, double *out_score,
                                 double *scratch_scores, double *scratch_models, int *lm_stat, int lm_schedule, double *record, int K,
                                 int *tie_stats, double tie_window, void *stream);

/* The key block of a sharded stream, in device memory (16 bytes).  seed: the generator key, as *seed of the _dseed entries.
 * cloud_base: the GLOBAL index of the launch's cloud 0.  A cloud then draws the same samples whichever launch serves it and at
 * whatever position: cloud b of a launch with base c gets the samples of cloud c + b of a launch with base 0.  reserved: unused (0). */
typedef struct {
    unsigned long long seed;
    int cloud_base;
    int reserved;
} ancsh_stream_key;

/* ancsh_ransac_single_rec_dseed / ancsh_ransac_joint_rec_dseed with the key block: the generator's problem index becomes
 * prob + key->cloud_base * K (stage A, prob = b * K + part) and prob + key->cloud_base * (K - 1) (stage B, prob = b * (K - 1) + joint);
 * stage B still adds 1 to the seed.  Only the generator's key moves: offsets, draws, scores, scratch and the record stay indexed by the
 * local prob, and explicit draws still override the generator.  So the fits of clouds [lo, hi) with cloud_base = lo equal rows [lo, hi)
 * of the whole batch's by-value fit (seed s, s + 1) byte for byte.  K is required (it is the problem count of one cloud): nprob must be
 * a multiple of K (stage A) / K - 1 >= 1 (stage B), below 2^20.  The draw keys stay clear of the sampler's tag bits 60..63 while
 * (cloud_base + B) * K < 2^20, B = the launch's clouds; cloud_base is in device memory, so that bound is the caller's to keep where it
 * writes the block (AncshPipeline.submit refuses larger bases).  The kernels are the by-value ones instantiated with a third key mode;
 * the by-value and _dseed instantiations are unchanged (profiles/r09_sharded_stream_isa_compare.txt).  key == NULL is refused. */
int ancsh_ransac_single_rec_dkey(int nprob, const int *off, const float *src, const float *tgt, float inlier_th, int niter,
                                 const int *draws, const ancsh_stream_key *key, int max_n, double *out_model,
                                 unsigned char *out_inliers, int *out_best, int *scratch_scores, float *scratch_quads, long rows,
                                 double *record, int K, int *tie_stats, float tie_window, void *stream);
int ancsh_ransac_joint_rec_dkey(int nprob, const int *rng0, const int *rng1, const float *src, const float *tgt,
                                const float *joint_dir, double inlier_th, int niter, const int *draws, const ancsh_stream_key *key,
                                int max_n, double *out_model, unsigned char *out_inliers, int *out_best, double *out_score,
                                double *scratch_scores, double *scratch_models, int *lm_stat, int lm_schedule, double *record, int K,
                                int *tie_stats, double tie_window, void *stream);

/* ancsh_ransac_joint_rec / _rec_dseed / _rec_dkey with a JOINT KIND per problem (ABI 14).  joint_kind (nprob) int32 in device memory,
 * problem p = b * (K - 1) + q as everywhere in stage B: ANCSH_JOINT_REVOLUTE (0) fits the revolute objective of the entries above
 * (objective_eval, :56-68: the two rotations agree on the joint direction, R0 u = R1 u), ANCSH_JOINT_PRISMATIC (1) the prismatic one
 * (objective_eval_r, :70-81, what joint_transformation_estimator(..., joint_type='prismatic') minimises, :150-152): the point rows are
 * the same, and the min(n0, n1) joint rows give way to three rows r0 - r1 of weight 1 between the two rotation VECTORS -- a slider
 * does not turn against its base.  Every hypothesis fit (3 * 6 + 3 = 21 rows) and the refit on the consensus set (3 (n0 + n1) + 3
 * rows) of a prismatic problem minimise it, with MINPACK's forward differences as for the revolute rows; scales, centring, the Kabsch
 * start, ftol, maxfev, the translations, the verifier and the score are shared.  Kinds may be mixed freely inside one call: the kind is
 * uniform per problem, a problem is a block index, so no lane ever diverges on it.
 *   - joint_kind == NULL, or all zeros: the bytes of the entry without it (record, model, masks, best, score, tie counts, lm_stat).
 *     With NULL the launches ARE that entry's; otherwise the same number of launches runs kernels that branch per block, whose
 *     revolute half is the same code (profiles/r14_pose_resource_usage_{before,after,diff}.txt: the kernels of the entries without a
 *     kind array keep their registers, scratch and occupancy).
 *   - a device array is never read by the host (no synchronisation, so the call can be captured): the kernels take ANY non-zero entry
 *     as prismatic.  The only valid host-side array is PINNED or REGISTERED host memory (hipHostMalloc / hipHostRegister, which the
 *     kernels can read): a plain pageable host pointer is not a valid argument -- the runtime reports it as unregistered memory, it
 *     cannot be told from a bad pointer and is not examined.  A pinned / registered array is checked before anything is launched, and an entry other
 *     than 0 / 1 is ANCSH_EINVAL with the offending index in ancsh_last_error().  Nothing traps or asserts on the device.
 *   - a prismatic problem does not read joint_dir[p]: it may hold NaN (a joint no point selects under
 *     ancsh_pose_joint_direction_pred) and the fit is finite all the same.  joint_dir itself must still be a valid (nprob, 3) array. */
#define ANCSH_JOINT_REVOLUTE 0
#define ANCSH_JOINT_PRISMATIC 1
int ancsh_ransac_joint_rec_kind(int nprob, const int *rng0, const int *rng1, const float *src, const float *tgt,
                                const float *joint_dir, double inlier_th, int niter, const int *draws, unsigned long long seed,
                                int max_n, double *out_model, unsigned char *out_inliers, int *out_best, double *out_score,
                                double *scratch_scores, double *scratch_models, int *lm_stat, int lm_schedule, double *record, int K,
                                int *tie_stats, double tie_window, const int *joint_kind, void *stream);
int ancsh_ransac_joint_rec_dseed_kind(int nprob, const int *rng0, const int *rng1, const float *src, const float *tgt,
                                      const float *joint_dir, double inlier_th, int niter, const int *draws,
                                      const unsigned long long *seed, int max_n, double *out_model, unsigned char *out_inliers,
                                      int *out_best, double *out_score, double *scratch_scores, double *scratch_models, int *lm_stat,
                                      int lm_schedule, double *record, int K, int *tie_stats, double tie_window, const int *joint_kind,
                                      void *stream);
int ancsh_ransac_joint_rec_dkey_kind(int nprob, const int *rng0, const int *rng1, const float *src, const float *tgt,
                                     const float *joint_dir, double inlier_th, int niter, const int *draws, const ancsh_stream_key *key,
                                     int max_n, double *out_model, unsigned char *out_inliers, int *out_best, double *out_score,
                                     double *scratch_scores, double *scratch_models, int *lm_stat, int lm_schedule, double *record, int K,
                                     int *tie_stats, double tie_window, const int *joint_kind, void *stream);

/* THE WHOLE FIT IN ONE CALL: ancsh_ransac_joint_rec* and ancsh_ransac_single_rec* of one batch, issued together on one stream, with
 * stage B's LM fits and stage A's refit in ONE kernel (no ABI bump: detected by their symbols).  Why: the LM launch is 64 waves of which
 * all but one are gone after a fifth of its duration, and with few hardware queues a batch's launches run one after another on one
 * in-order queue -- stage A's refit (one workgroup per part, sharing nothing with stage B but the partition) then held that queue for a
 * launch of its own.  Here it rides behind the LM blocks of the same grid.  Launches, in order: soa_quads, score_sreg (stage A scoring),
 * joint_init, pose_lm_finish_a (LM fits || stage A refit), joint_model, joint_verify, joint_finish -- seven where the two calls issue eight.
 *   - The arguments are the union of the two entries': the `_a` ones are ancsh_ransac_single_rec*'s (nprob_a = b * K problems, off,
 *     inlier_th_a, niter_a, draws_a (nprob_a, niter_a, 3), key_a, outputs, scratch_scores_a, scratch_quads, rows, tie_stats_a,
 *     tie_window_a), the `_b` ones ancsh_ransac_joint_rec*'s (nprob_b = b * (K - 1) problems, rng0 / rng1, joint_dir, inlier_th_b, niter_b,
 *     draws_b (nprob_b, niter_b, 6), key_b, outputs, both scratch arrays, lm_stat, lm_schedule, tie_stats_b, tie_window_b); src, tgt, max_n
 *     (<= 3072, stage B's bound), record and K are shared.  key_a / key_b: the two calls' own key arguments -- by value the pair (s, s + 1)
 *     PoseSolver.solve passes, for _dseed / _dkey the same pointer twice (stage B adds 1 to the seed itself).
 *   - Every output byte equals what the two calls write: the record, both models, masks, winners, scores, tie counts, lm_stat.  The LM
 *     blocks run ransac_joint_lm_kernel's code, four chunks of hypotheses per 256-thread block (the chunk size follows the launch size as
 *     there); the refit blocks run ransac_single_finish_kernel's code.  tests/test_pose_fused_launch_gpu.py.
 *   - Every argument check of both entries runs before anything is launched (same messages).  nprob_a == 0 and nprob_b == 0: nothing is
 *     launched, ANCSH_OK.  One of them 0: the other stage's existing launches.  lm_schedule == ANCSH_LM_LATENCY (the eight-lane LM
 *     kernel): the two calls' eight launches, stage B first.  scratch_quads == NULL (or a threshold outside the scalar-register kernel's
 *     range): one scoring launch instead of soa_quads + score_sreg, as in ancsh_ransac_single_rec.
 *   - the _kind forms take joint_kind as ancsh_ransac_joint_rec_kind does (NULL = the form without it). */
int ancsh_pose_fit_rec(int nprob_a, const int *off, const float *src, const float *tgt, float inlier_th_a, int niter_a,
        const int *draws_a, unsigned long long key_a, int max_n, double *out_model_a, unsigned char *out_inliers_a, int *out_best_a,
        int *scratch_scores_a, float *scratch_quads, long rows, int *tie_stats_a, float tie_window_a, int nprob_b, const int *rng0,
        const int *rng1, const float *joint_dir, double inlier_th_b, int niter_b, const int *draws_b, unsigned long long key_b,
        double *out_model_b, unsigned char *out_inliers_b, int *out_best_b, double *out_score_b, double *scratch_scores_b,
        double *scratch_models_b, int *lm_stat, int lm_schedule, int *tie_stats_b, double tie_window_b, double *record, int K,
        void *stream);
int ancsh_pose_fit_rec_dseed(int nprob_a, const int *off, const float *src, const float *tgt, float inlier_th_a, int niter_a,
        const int *draws_a, const unsigned long long * key_a, int max_n, double *out_model_a, unsigned char *out_inliers_a, int *out_best_a,
        int *scratch_scores_a, float *scratch_quads, long rows, int *tie_stats_a, float tie_window_a, int nprob_b, const int *rng0,
        const int *rng1, const float *joint_dir, double inlier_th_b, int niter_b, const int *draws_b, const unsigned long long * key_b,
        double *out_model_b, unsigned char *out_inliers_b, int *out_best_b, double *out_score_b, double *scratch_scores_b,
        double *scratch_models_b, int *lm_stat, int lm_schedule, int *tie_stats_b, double tie_window_b, double *record, int K,
        void *stream);
int ancsh_pose_fit_rec_dkey(int nprob_a, const int *off, const float *src, const float *tgt, float inlier_th_a, int niter_a,
        const int *draws_a, const ancsh_stream_key * key_a, int max_n, double *out_model_a, unsigned char *out_inliers_a, int *out_best_a,
        int *scratch_scores_a, float *scratch_quads, long rows, int *tie_stats_a, float tie_window_a, int nprob_b, const int *rng0,
        const int *rng1, const float *joint_dir, double inlier_th_b, int niter_b, const int *draws_b, const ancsh_stream_key * key_b,
        double *out_model_b, unsigned char *out_inliers_b, int *out_best_b, double *out_score_b, double *scratch_scores_b,
        double *scratch_models_b, int *lm_stat, int lm_schedule, int *tie_stats_b, double tie_window_b, double *record, int K,
        void *stream);
int ancsh_pose_fit_rec_kind(int nprob_a, const int *off, const float *src, const float *tgt, float inlier_th_a, int niter_a,
        const int *draws_a, unsigned long long key_a, int max_n, double *out_model_a, unsigned char *out_inliers_a, int *out_best_a,
        int *scratch_scores_a, float *scratch_quads, long rows, int *tie_stats_a, float tie_window_a, int nprob_b, const int *rng0,
        const int *rng1, const float *joint_dir, double inlier_th_b, int niter_b, const int *draws_b, unsigned long long key_b,
        double *out_model_b, unsigned char *out_inliers_b, int *out_best_b, double *out_score_b, double *scratch_scores_b,
        double *scratch_models_b, int *lm_stat, int lm_schedule, int *tie_stats_b, double tie_window_b, double *record, int K,
        const int *joint_kind, void *stream);
int ancsh_pose_fit_rec_dseed_kind(int nprob_a, const int *off, const float *src, const float *tgt, float inlier_th_a, int niter_a,
        const int *draws_a, const unsigned long long * key_a, int max_n, double *out_model_a, unsigned char *out_inliers_a, int *out_best_a,
        int *scratch_scores_a, float *scratch_quads, long rows, int *tie_stats_a, float tie_window_a, int nprob_b, const int *rng0,
        const int *rng1, const float *joint_dir, double inlier_th_b, int niter_b, const int *draws_b, const unsigned long long * key_b,
        double *out_model_b, unsigned char *out_inliers_b, int *out_best_b, double *out_score_b, double *scratch_scores_b,
        double *scratch_models_b, int *lm_stat, int lm_schedule, int *tie_stats_b, double tie_window_b, double *record, int K,
        const int *joint_kind, void *stream);
int ancsh_pose_fit_rec_dkey_kind(int nprob_a, const int *off, const float *src, const float *tgt, float inlier_th_a, int niter_a,
        const int *draws_a, const ancsh_stream_key * key_a, int max_n, double *out_model_a, unsigned char *out_inliers_a, int *out_best_a,
        int *scratch_scores_a, float *scratch_quads, long rows, int *tie_stats_a, float tie_window_a, int nprob_b, const int *rng0,
        const int *rng1, const float *joint_dir, double inlier_th_b, int niter_b, const int *draws_b, const ancsh_stream_key * key_b,
        double *out_model_b, unsigned char *out_inliers_b, int *out_best_b, double *out_score_b, double *scratch_scores_b,
        double *scratch_models_b, int *lm_stat, int lm_schedule, int *tie_stats_b, double tie_window_b, double *record, int K,
        const int *joint_kind, void *stream);

/* Batched estimateSimilarityUmeyama (lib/aligning.py:580-622; GT poses of evaluation/compute_gt_pose.py:87).
 * Problem p = rows [off[p], off[p+1]) of src/tgt.  out (nprob,32) float64: Scales(3) | Rotation(9, the
 * reference's TRANSPOSED matrix) | Translation(3) | OutTransform (4x4 row-major, 16) | pad(1). */
int ancsh_umeyama(int nprob, const int *off, const float *src, const float *tgt, double *out, void *stream);

/* Batched estimateSimilarityTransform (lib/aligning.py:17-32 with set_config :88-103, getRANSACInliers :485-507,
 * evaluateModel :540-547): 5-point Umeyama RANSAC, niter (reference: 100, max 128) iterations with the reference's
 * sequential bookkeeping (strictly better inlier ratio wins; stop once the best residual < PassThreshold/100; the
 * count_nonzero-of-indices quirk that never counts point 0), then Umeyama on the winner's inliers.
 * draws (nprob, niter, 5) int32 (the reference draws np.random.randint(n, size=5), :490) or NULL (device generator).
 * out (nprob,32) float64 laid out as ancsh_umeyama's, out[31] = BestInlierRatio; status (nprob): 0 ok, 1 = the reference
 * returns 4 x None (BestInlierRatio < 0.1; out row is NaN), -1 empty problem. */
int ancsh_estimate_similarity_transform(int nprob, const int *off, const float *src, const float *tgt, int niter,
                                        const int *draws, unsigned long long seed, double *out, int *status, void *stream);

/* iou_3d of lib/d3_utils.py:55-69 (per-part amodal box IoU of evaluation/compute_miou.py:212-225) for npairs box pairs in one
 * launch: bbox1, bbox2 (npairs, 8, 3) float64 corners in the reference's get_3d_bbox order; a nres^3 numpy.linspace grid over
 * the joint axis-aligned bounds; iou[p] = |inside both| / |inside either| (1.0 when the union is empty).  counts (npairs, 2)
 * int64 {intersection, union} is optional (NULL to skip). */
int ancsh_iou_3d(int npairs, int nres, const double *bbox1, const double *bbox2, double *iou, long *counts, void *stream);

/* Joint parameters from the per-point heads, evaluation/eval_joint_params.py:143-199, for b clouds in one launch (float32
 * inputs with the .h5 record's layouts, (b, n, .) row-major):
 *   gocs (b,n,gocs_channels) global NOCS, gocs_channels = 3*K (per part: a point reads its predicted part's triple) or 3;
 *   nocs (b,n,3K) part NOCS; mask (b,n,K) part scores (np.argmax = first maximum); heatmap (b,n); unitvec, joint_axis (b,n,3);
 *   joint_cls (b,n) int32 joint class per point (argmax of index_per_point / joint_cls_gt).
 * st (b,K,4) float64: scale_j = std(mean(y,1)) / std(mean(x,1)) and translation_j = mean(y - scale_j x, 0) over the points of
 *   predicted part j (x global, y part NOCS; :160-171), NaN for an empty part; nocs and st may BOTH be NULL to skip.
 * joint (b,K-1,6) float64: [joint point (3) | joint axis (3)] of joint j = 1..K-1 in global-NOCS space: per-channel median over
 *   the points of joint class j of  gocs + unitvec * (1 - heatmap) * 0.2  and of joint_axis (:176-187); axis_mean != 0 = the
 *   ground-truth variant (:189-199): the axis is the float32 mean instead of the median.  mask may be NULL when gocs_channels == 3.
 * Element arithmetic in float32 in numpy's order; medians are exact selections; NaN rows for a joint class without points.
 * numpy's rules at the edges: a NaN in a mask row is that point's label (np.argmax: the first maximum, or the first NaN); a channel
 * with a NaN vote has a NaN median (np.median; +-inf votes sort as numbers, an even count's -inf and +inf middle gives NaN); the std is
 * taken in two passes, so a part whose row means are all the same float32 value has std exactly 0 and a scale of inf or NaN. */
int ancsh_joint_params(int b, int n, int K, int gocs_channels, int axis_mean, const float *gocs, const float *nocs,
                       const float *mask, const float *heatmap, const float *unitvec, const float *joint_axis,
                       const int *joint_cls, double *st, double *joint, void *stream);

/* Amodal-box extents and boundaries of the predicted parts: the per-part block evaluation/compute_miou.py:196-208 and
 * evaluation/eval_pose_err.py:253-268 run one frame and one part at a time.  nocs (b,n,nocs_channels) float32 with 3K channels
 * (part j reads its own slot) or 3; mask (b,n,K) float32 (a point belongs to the part of its FIRST maximum, np.argmax); P rows of ldp
 * floats whose first three are the point; pose0 (b,12) float64 = part 0's fitted rotation row-major (9) and translation (3), rounded
 * to float32 inside like the reference's compose_rt.  Outputs per (cloud, part): scale_pred (b,K,3) float32 = 2 * max |nocs - 0.5|,
 * dynam (b,K) float64 = min x of the part's points in part 0's frame (the "dynamic boundary"), count (b,K) points of the part
 * (0 -> NaN outputs; the reference drops such a frame through its bare except).  K <= 8.  A NaN in a mask row is that point's label
 * (np.argmax: the first NaN ranks above every number). */
int ancsh_part_extents(int b, int n, int K, int nocs_channels, const float *nocs, const float *mask, const float *P, int ldp,
                       const double *pose0, float *scale_pred, double *dynam, int *count, void *stream);

/* Articulation block of a streamed batch, one launch after the pose fit and the record poison (ABI 11): the pred side of
 * evaluation/compute_miou.py:196-222 (amodal boxes) and evaluation/eval_joint_params.py:143-220 (joints in camera space), fused.
 * Inputs (b,n,.) float32 row-major, the two networks' heads:
 *   ANCSH: gocs (gocs_channels = 3K or 3), nocs (3K) part NOCS, mask (K) = W, heatmap (1), unitvec (3), joint_axis (3), joint_index (joint_channels)
 *     = index_per_point (joint class = its first argmax, np.argmax; joint j >= joint_channels has no points);
 *   NPCS: npcs_nocs (3K), npcs_mask (K) = W;  record (b,K,26) float64: the pose record, nonlinear R_j 13..21 (row-major), s_j 22, t_j 23..25.
 * art (b,K,12) float64, row j:
 *   0..2   s_j * scale_pred_j, scale_pred_j = 2 max |npcs_nocs_j - 0.5| over the points whose npcs_mask first maximum is j  (:196-200, 214-217)
 *   3..5   s_j R_j (1/2,1/2,1/2) + t_j: the centre of get_3d_bbox(scale, shift=1/2) (lib/d3_utils.py:8) in camera space  (:217-222)
 *   6..8   (j >= 1) pivot R_0 (s_0 (p_j s2 + t2)) + t_0: p_j = per-channel median over joint class j of gocs + unitvec (1 - heatmap) 0.2,
 *          (s2, t2) = part 0's similarity global -> part NOCS (ancsh_joint_params' st row 0)     (eval_joint_params.py:143-187, 214-219)
 *   9..11  (j >= 1) axis R_0 a_j: a_j = per-channel median of joint_axis over the same points, not normalised        (:176-187, 220)
 *   row 0's 6..11 NaN.  An empty part / joint class: NaN in its own columns; a NaN in part 0's nonlinear pose (a poisoned record):
 *   the cloud's whole block NaN.  K = 1: box columns only.  Labels, medians and the similarity follow ancsh_joint_params' rules: a NaN
 *   in a mask or joint_index row is the label (first NaN), a NaN vote makes its channel's median NaN, the std is taken in two passes.
 * Optional (NULL to skip), bit-equal to the offline kernels: joint_nocs (b,K-1,6) = ancsh_joint_params' joint, st0 (b,4) = its st row 0
 * (NaN for K = 1), extent (b,K,3) float32 = ancsh_part_extents' scale_pred.  K <= 8, n <= ANCSH_ARTICULATION_MAX_N (LDS-resident medians:
 * 6 columns of the next power of two of n floats). */
#define ANCSH_ARTICULATION_MAX_N 4096
int ancsh_articulation_rec(int b, int n, int K, int gocs_channels, int joint_channels, const float *gocs, const float *nocs,
                           const float *mask, const float *heatmap, const float *unitvec, const float *joint_axis,
                           const float *joint_index, const float *npcs_nocs, const float *npcs_mask, const double *record,
                           double *art, double *joint_nocs, double *st0, float *extent, void *stream);

/* Joint states of a streamed batch, one launch behind ancsh_articulation_rec (no new ABI number: callers detect it by its symbol): the
 * pred side of evaluation/eval_pose_err.py:304-321 -- the relative rotation R_0^T R_j and the relative translation of every child part
 * against part 0, as t_j - t_0 (:318) and as the boundary slide dynam_j - canon_j (:263-266, 320) -- per cloud, one workgroup each.
 * P (b,n,.) float32 rows of ldp floats whose first three are the sampled point; npcs_nocs (b,n,3K), npcs_mask (b,n,K) float32: the NPCS
 * heads; record (b,K,26) float64: nonlinear R_j 13..21 (row-major), s_j 22, t_j 23..25; art (b,K,12) float64 as ancsh_articulation_rec
 * wrote it.  wide (b,K,20) float64, row j:
 *   0..11  art[b][j][0..11], bit for bit (NaN payloads included)
 *   12     angle_j = atan2(|v|, c) in degrees, c = (tr Rrel - 1) / 2, v = 1/2 (Rrel[2][1] - Rrel[1][2], Rrel[0][2] - Rrel[2][0],
 *          Rrel[1][0] - Rrel[0][1]), Rrel = R_0^T R_j in float64: rot_diff_degree(I, Rrel) (lib/d3_utils.py:144-148), well conditioned at
 *          0 and 180 degrees; R_0 = R_j gives exactly 0
 *   13     atan2(v . a, c) in degrees, a = R_0^T u, u = art[9..11] / |art[9..11]|: the angle signed about the joint axis (NaN for a NaN
 *          or zero axis)
 *   14..16 t_j - t_0 in camera space (:318)
 *   17     (t_j - t_0) . u, the slide along the joint axis (NaN with a NaN axis)
 *   18     dynam_j - canon_j in float64: dynam_j = ancsh_part_extents' dynam on P and npcs_mask with pose0 = [R_0 | t_0] of the record
 *          (bit-equal), canon_j = - scale_pred_j[0] / 2 + 0.5 in float32 with ancsh_part_extents' scale_pred on npcs_nocs (bit-equal);
 *          row 0 gets its own; NaN for a part without points
 *   19     the points of part j (ancsh_part_extents' count) as a double, every row
 * Row 0's 12..17 are NaN.  A NaN in part 0's nonlinear pose (record columns 13..25 of row 0): 12..18 of every row NaN; a NaN in part j's:
 * row j's 12..18 NaN.  K = 1: row 0 only.  1 <= K <= 8, n >= 1, ldp >= 3; b == 0 launches nothing. */
int ancsh_joint_state_rec(int b, int n, int K, const float *P, int ldp, const float *npcs_nocs, const float *npcs_mask,
                          const double *record, const double *art, double *wide, void *stream);

/* Fit quality of a pose record, one launch behind the fit and the record poison (no new ABI number: callers detect it by its symbol):
 * what the reference prints per part and drops (evaluation/parallel_ancsh_pose.py:273, 311, 322) and what its verifiers
 * (single_transformation_verifier :48-54, joint_transformation_verifier :186-194) say about the poses the record holds.
 * off (b*K+1) int32, src / tgt (rows,3) float32: ancsh_pose_partition's packed rows, part (c,j) = rows [off[cK+j], off[cK+j+1]), src the
 * point's own part-NOCS triple, tgt the sampled point; record (b,K,26) float64, read as it stands (after the poison); best_a (b*K,2)
 * int32 = ancsh_ransac_single*'s out_best, score_b (b*(K-1)) float64 = ancsh_ransac_joint*'s out_score: either may be NULL, its column
 * is then NaN.  wide (b,K,39) float64, row (c,j):
 *   0..25  record[c][j][0..25], bit for bit (NaN payloads included)
 *   26     n_j = off[cK+j+1] - off[cK+j], the points of the part
 *   27     best_a[cK+j][1], the stage-A winner's consensus count (:273's ninliers)
 *   28..32 the baseline pose (columns 0..12 = R row-major, s, t): points with rho < inlier_th under this REFIT pose, then the mean, the
 *          RMS, the median (np.median: the middle order statistic, or (a + b) / 2 of the two middle ones) and the max of rho over all n_j
 *          points
 *   33     score_b of the joint fit that produced this row's nonlinear pose: joint 1's for row 0, joint j's for row j >= 1; NaN for K = 1
 *   34..38 the nonlinear pose (columns 13..25): the same five numbers (K = 1: computed from 13..25 like any other)
 * rho of a point, float64 (src, tgt promoted), evaluated as written, no contraction:
 *   y_c = (R_c0 x_0 + R_c1 x_1) + R_c2 x_2;  r_c = (tgt_c - s y_c) - t_c;  rho = sqrt((r_0^2 + r_1^2) + r_2^2)
 * Counts, medians and maxima are exact; the sums behind mean and RMS are added in a fixed order (the same bytes every run, whatever b and
 * wherever the part lies in the batch).  n_j = 0: 28..32 and 34..38 NaN.  A NaN among a pose's 13 numbers: that pose's five columns NaN.
 * A part longer than ANCSH_FIT_QUALITY_MAX_N points is clamped IN THE KERNEL (off lives on the device and is never read by the host, so the
 * call stays capturable): its row keeps the true n_j in column 26 and gets NaN in 28..32 and 34..38.
 * 1 <= K <= 16, inlier_th finite and > 0; b == 0 launches nothing. */
#define ANCSH_FIT_QUALITY_MAX_N 8192      /* the residuals of one pose stay in LDS: the fit's own bound on a part */
int ancsh_fit_quality_rec(int b, int K, const int *off, const float *src, const float *tgt, const double *record, double inlier_th,
                          const int *best_a, const double *score_b, double *wide, void *stream);

/* Errors of a pose record against ground truth, one launch behind the fit (and, if built, the fit-quality launch; no new ABI number:
 * callers detect it by its symbol).  It replaces, per frame and part, the numbers the reference's offline evaluation reports: rpy_err /
 * xyz_err / scale_err of both poses (evaluation/parallel_ancsh_pose.py, the end of solver_ransac_nonlinear), the 3-D IoU of the amodal
 * boxes (evaluation/compute_miou.py:150-229 with lib/d3_utils.py:14-69) and the relative rotation and translation error per joint
 * (evaluation/eval_pose_err.py:279-338, its ground-truth side :304-326; ancsh_joint_state_rec is the pred side).
 * P (b,n,.) float32 rows of ldp floats whose first three are the sampled point; npcs_nocs (b,n,3K), npcs_mask (b,n,K) float32: the NPCS
 * heads the record was fitted on; record (b,K,ld) float64 rows, ld = 26 (the record) or 39 (ancsh_fit_quality_rec's wide record): the
 * baseline pose in 0..12 and the nonlinear pose in 13..25, each R (9, row-major) | s | t (3).
 * gt (b,K,19) float64, row (c,j), in the space the fit works in (the sampled cloud P = xyz * norm_factor, as compute_gt_pose produces it):
 *   0..8   R_gt, row-major (pn_gt[...]['rt']['gt'][j][:3,:3])
 *   9      s_gt (pn_gt[...]['scale']['gt'][j])
 *   10..12 t_gt
 *   13..15 NOCS extent of the ground-truth box (bbox3d_all[ins][j][1][0] - bbox3d_all[ins][j][0][0], compute_miou.py)
 *   16..18 translation of the NAOCS ground-truth pose (gn_gt[...]['rt']['gt'][j][:3,3]); only column ld+10 reads it
 * wide (b,K,ld+12) float64, row (c,j): columns 0..ld-1 = the input row bit for bit (NaN payloads included), then
 *   ld+0..2  baseline pose: rpy_err = rot_diff_degree(R, R_gt) in degrees (lib/d3_utils.py:144-148: arccos((tr(R R_gt^T) - 1) / 2) mod
 *            2 pi, / pi * 180; no clamp, like the reference: a trace above 3 gives NaN); xyz_err = |t - t_gt|; scale_err = |s - s_gt|
 *   ld+3     baseline pose: 3-D IoU of the ground-truth box against the predicted box (below)
 *   ld+4     baseline pose, row j >= 1: rot_diff_degree(R_gt0^T R_gtj, R_0^T R_j) (eval_pose_err.py:304-312, 327); row 0: NaN
 *   ld+5..9  nonlinear pose: the same five numbers
 *   ld+10    nonlinear pose, row j >= 1: |(t_naocs_j - t_naocs_0) - d_j R_0[:,0]| (:316-326), d_j = dynam_j - canon_j bit-equal to
 *            ancsh_joint_state_rec's column 18, R_0 = the record's nonlinear part-0 rotation; row 0: NaN
 *   ld+11    points of predicted NPCS part j (first maximum of npcs_mask; ancsh_part_extents' count) as a double
 * float64 evaluated as written, no contraction: tr(A B^T) = (d_0 + d_1) + d_2 with d_a = (A_a0 B_a0 + A_a1 B_a1) + A_a2 B_a2;
 * (A^T B)_ac = (A_0a B_0c + A_1a B_1c) + A_2a B_2c; norms sqrt((x^2 + y^2) + z^2).
 * 3-D IoU: scale_pred_j = 2 max |npcs_nocs_j - 0.5| over the part's points, float32, bit-equal to ancsh_part_extents; both boxes are
 * get_3d_bbox(extent, shift = 1/2) * s taken through . R^T + t -- corner = ((sign * (extent / 2) + 1/2) * s), then
 * ((R_c0 x + R_c1 y) + R_c2 z) + t_c -- with the predicted R and t rounded to float32 first (the reference's compose_rt) and the
 * ground-truth pose as given; then iou_3d (lib/d3_utils.py:55-69): an nres^3 numpy.linspace grid (the reference uses 50) over the joint
 * axis-aligned bounds, |inside both| / |inside either|, 1 when the union is empty; grid coordinates and inside tests are ancsh_iou_3d's.
 * Counts are integers: the same bytes every run and wherever the cloud lies in the batch.
 * NaN rules: a NaN among a pose's 13 numbers blanks that pose's five columns (and, nonlinear, ld+10); a NaN in part 0's pose blanks that
 * pose's relative columns (ld+4, or ld+9 and ld+10) of every row; a NaN in a gt entry blanks every column that reads it (rpy_err: 0..8;
 * xyz_err: 10..12; scale_err: 9; the IoU: 0..15; the relative rotation: 0..8 of rows 0 and j; ld+10: 16..18 of rows 0 and j) -- an all-NaN
 * gt row is how a frame without ground truth travels; a part without predicted points gets NaN in ld+3, ld+8 and ld+10.  K = 1: row 0
 * only.  1 <= K <= 8, n >= 1, ldp >= 3, ld in {26, 39}, 2 <= nres <= 64; b == 0 launches nothing. */
int ancsh_gt_error_rec(int b, int n, int K, int nres, const float *P, int ldp, const float *npcs_nocs, const float *npcs_mask,
                       const double *record, int ld, const double *gt, double *wide, void *stream);

/* What a streamed batch's PER-POINT ground truth says about it, one launch behind the articulation launches (ancsh_articulation_rec and,
 * if built, ancsh_joint_state_rec; no new ABI number: callers detect it by its symbol): the test-time losses of both networks
 * (lib/network.py:257-316 over lib/loss.py: the numbers of test_loss.txt) and step 5 of evaluation.sh, each joint's axis angle error and
 * line-to-line distance in camera space (evaluation/eval_joint_params.py:189-256).  One workgroup per cloud; every size is an argument or
 * read from device memory, nothing is allocated and the host never waits: capturable.
 * rows (capacity, nchan = 18) float32: the raw rows of the batch, dataset.pack_cloud's layout
 *   x y z | cls | nocs_p 3 | nocs_g 3 | heatmap | unitvec 3 | orient 3 | joint_cls;
 * offsets (b+1) int32 on the device: cloud c owns rows [offsets[c], offsets[c+1]); perm (b,n) int32: ancsh_input_sample_stream*'s perm_out.
 * Sampled point i of cloud c is raw row offsets[c] + perm[c][i] % n_raw, and its channels 3..17 are read by ancsh_input_sample's rules:
 * cls_gt and joint_cls_gt = the C truncation to int32, mask_array = the one-hot of int8(cls) with numpy's negative-index rule,
 * joint_cls_mask = joint_cls > 0, nocs_gt = nocs_p, nocs_gt_g = nocs_g.
 * The ANCSH heads (b,n,.) float32: W (K), nocs (3K), gocs (gocs_channels = 3K or 3), heatmap (1), unitvec (3), joint_axis (3), joint_index
 * (joint_channels); the NPCS heads: npcs_W (K), npcs_nocs (3K).  art (b,K,ld_art) float64, ld_art = 12 (ancsh_articulation_rec's block) or
 * 20 (ancsh_joint_state_rec's): the predicted joint j in camera space, pivot 6..8 and axis 9..11.  frame (b,13) float64 = [R (9,
 * row-major) | s | t (3)] of the ground-truth NAOCS pose of part 0 (gn_gt[...]['rt']['gt'][0], gn_gt[...]['scale']['gt'][0]).  record
 * (b,K,ld) float64 rows, ld = 26 (the record), 39 (ancsh_fit_quality_rec's), 38 or 51 (ancsh_gt_error_rec's behind either).  type_l: 0 =
 * L2, 1 = L1 (coord_regress_loss).
 * wide (b,K,ld+21) float64, row (c,j): columns 0..ld-1 = the input row bit for bit (NaN payloads included), then
 *   ld+0     row j >= 1: angle_err = axis_diff_degree(l_gt, art[9..11]) in degrees (lib/d3_utils.py:137-142: no clamp, min(a, 180 - a))
 *   ld+1     row j >= 1: dist_err = dist_between_3d_lines(p_gt, l_gt, art[6..8], art[9..11]) (:165-174)
 *   ld+2..4  row j >= 1: p_gt = R (s p) + t, the ground-truth joint point in camera space (eval_joint_params.py:224-231)
 *   ld+5..7  row j >= 1: l_gt = R l, the ground-truth joint axis in camera space, not normalised
 *   ld+8     miou_loss[j] of the ANCSH network;  ld+9  miou_loss[j] of the NPCS network
 *   ld+10    sampled points with cls_gt == j;  ld+11  sampled points with joint_cls_gt == j
 *   ld+12..19 the cloud's ANCSH nocs, gocs, heatmap, unitvec, orient and index[0..2] losses, the same bits on every row
 *   ld+20    the cloud's NPCS nocs_loss, the same bits on every row
 * The losses are ancsh_test_losses' 5 + K + 3 numbers on the gathered tensors, BIT-EQUAL (float32 values held as doubles): the same
 * statements and the same accumulation order -- thread tid of 256 takes points tid, tid + 256, ..., float64 partial sums, xor-shuffle
 * wave sums, four waves added in order.  gocs_loss is NaN when gocs_channels == 3 != 3K (no per-part global NOCS head), the index losses when joint_channels != 3.
 * (p, l) of joint j in global NOCS are ancsh_joint_params' axis_mean = 1 numbers on the gathered nocs_gt_g, heatmap_gt, unitvec_gt,
 * orient_gt, joint_cls_gt with gocs_channels = 3, BIT-EQUAL: p = the per-channel exact median of nocs_g + unitvec * (1 - heatmap) * 0.2
 * over the points of joint class j (float32, numpy's order), l = the float32 mean of their orientations in point order (:189-199).
 * joint_gt (b,K-1,6) float64, optional (NULL to skip): [p | l] of joints 1..K-1 before the camera transform.
 * Camera space and errors in float64, evaluated as written, no contraction: x_k = ((R_k0 a_0 + R_k1 a_1) + R_k2 a_2) [+ t_k]; dot and
 * squared norms (x^2 + y^2) + z^2; angle = acos(dot / (|l_gt| |l|)) * 180 / pi; dist = |((l_gt x l) . (p_gt - p))| / |l_gt x l|.
 * NaN rules: row 0's ld+0..7 are NaN; a joint class without ground-truth points has ld+0..7 NaN; a NaN in frame blanks ld+0..7 of the
 * cloud; a NaN in art[j][6..11] (an empty predicted joint class, a poisoned record) blanks ld+0 and ld+1 of row j.  The losses are
 * whatever the arithmetic gives.  A cloud whose offsets are empty or reach outside capacity (the host refuses both) gets NaN in all 21
 * columns.  A cloud never changes a neighbour's bytes.  K = 1: row 0 only.
 * 1 <= K <= 8, nchan == 18, 1 <= n <= ANCSH_ARTICULATION_MAX_N (the votes' six columns stay in LDS), ld in {26, 39, 38, 51}, ld_art in
 * {12, 20}, 0 <= capacity < 2^30; b == 0 launches nothing. */
int ancsh_point_gt_rec(int b, int n, int K, int nchan, const float *rows, long capacity, const int *offsets, const int *perm,
                       int gocs_channels, int joint_channels, const float *W, const float *nocs, const float *gocs, const float *heatmap,
                       const float *unitvec, const float *joint_axis, const float *joint_index, const float *npcs_W,
                       const float *npcs_nocs, const double *art, int ld_art, const double *frame, const double *record, int ld, int type_l,
                       double *wide, double *joint_gt, void *stream);

/* The per-point ground truth itself, built from annotated clouds in ONE launch in front of the streaming sampler (no new ABI number:
 * callers detect it by its symbol): the arithmetic of lib/dataset.py:434-700 behind the two h5py lookups -- create_data_shape2motion
 * (:490-547) and create_data_mobility (:603-699) -- and the sapien rotation of :371-379, which the reference runs per part in numpy on the
 * host.  Cloud b owns rows [offsets[b], offsets[b+1]) of src (capacity x 7 float32) and of rows (capacity x 18 float32, the layout
 * ancsh_point_gt_rec reads); offsets (nclouds + 1) int32 on the device.  A source row is [x y z | c (3) | part]: a camera point
 * (gt_points), its canonical coordinates (gt_coords) and the index of its group in parts_map.  rig (nclouds, rig_ld) float64, rig_ld =
 * ANCSH_RIG_WIDTH(K), per cloud:
 *   [0] thres_r   [1] the default joint label (0 shape2motion :539, K sapien :672)   [2] 0: a line entry selects h < thres_r (:543),
 *   1: h <= thres_r (:683)   [3] non-zero: rotate by R   [4..12] R, row-major (the identity, or the base joint's euler_matrix :371-374)
 *   [13..15] corner0[0]   [16..18] norm_factors[0] per axis   [19..21] 0.5 * (corner0[1] - corner0[0]) * norm_factors[0]
 *   then per part j, ANCSH_RIG_PART(K) = 15 + 9K wide, at ANCSH_RIG_HEAD + j * ANCSH_RIG_PART(K):
 *   [0..2] sub_j (0, or link_xyz[j][0] :613)   [3..5] corner_j[0]   [6..8] factor_j per axis   [9..11] 0.5 * (corner_j[1] - corner_j[0]) *
 *   factor_j, all of norm_*[j+1]   [12] cls_out   [13] jcls_out, < 0: not set   [14] n_j entries   [15 + 9k ..] entry k:
 *   [P0 (3) | l (3) | id | kind (0 line, 1 constant, 2 origin) | |l|^2].
 * For a row of part j, float64 throughout (the seven float32 inputs widened), evaluated as written, no contraction:
 *   cc = c - sub_j;  g0 = ((cc - corner0[0]) * nf0 + 0.5) - tail0 (:498 / :625);  p0 likewise with part j's own three vectors (:494 / :621);
 *   heatmap = 0, unitvec = 0, orient = 0, jcls = rig[1]; then entries k = 0 .. n_j - 1 in order, a later one overwriting an earlier one:
 *     line: d = g0 - P0, off = ((d0 l0 + d1 l1) + d2 l2) * l / |l|^2 - d (lib/d3_utils.py:192-203);  constant: off = 0.5 * thres_r (x3, :633-635);
 *     origin: the line's formula with d = 0 - P0, and the entry reaches only the part's FIRST row -- the cloud's first row or one whose
 *     predecessor holds another part value.  This is what the reference computes for a sapien revolute joint: :638 measures the NAOCS
 *     origin, not the part's points, so the offset is one (1, 3) row and np.where (:683) can name index 0 of the part only;
 *     h = sqrt((off0^2 + off1^2) + off2^2), u = off / (h + 1e-7);  selected when h < (or <=) thres_r, a constant entry when h > 0; a NaN h
 *     (a zero axis) selects nothing;  selected: heatmap = 1 - h / thres_r, unitvec = u, orient = l, jcls = id;
 *   cls = cls_out, joint_cls = jcls_out if set (sapien relabels the whole part, :697-699) else jcls;
 *   rig[3] set: nocs_p = R (p0 - 0.5) + 0.5, nocs_g = R (g0 - 0.5) + 0.5, unitvec = R unitvec, orient = R orient, each row of R summed
 *   (x + y) + z; the heat-map is that of the unrotated g0, as in the reference.
 * rows[r] = [x y z bit for bit | cls | nocs_p | nocs_g | heatmap | unitvec | orient | joint_cls], every value rounded to float32 once, as
 * the reference's .astype(np.float32) rounds its float64 arrays.  A row whose part is not an integer in [0, K) never indexes the rig: cls =
 * joint_cls = -1 and NaN in the 13 columns between.  A non-finite c poisons its own row only.  Rows outside [offsets[0], offsets[nclouds])
 * are left untouched, and so is a cloud whose rows are empty or outside [0, capacity).  Deterministic byte for byte, no atomics.
 * Graph-capturable: the grid depends on (capacity, nclouds) only, every cloud size is read from device offsets; no host sync, no
 * allocation.  nclouds == 0 launches nothing.  Checked before any launch: 0 <= nclouds <= 65535, 1 <= K <= 8, rig_ld ==
 * ANCSH_RIG_WIDTH(K), 0 <= capacity < 2^30, null pointers. */
#define ANCSH_RIG_ROT 4
#define ANCSH_RIG_GMAP 13
#define ANCSH_RIG_HEAD 22
#define ANCSH_RIG_ENTRY 9
#define ANCSH_RIG_PART(K) (15 + ANCSH_RIG_ENTRY * (K))
#define ANCSH_RIG_WIDTH(K) (ANCSH_RIG_HEAD + (K) * ANCSH_RIG_PART(K))
int ancsh_point_gt_build(int nclouds, int K, const float *src, long capacity, const int *offsets, const double *rig, int rig_ld,
                         float *rows, void *stream);

/* The ground-truth poses of a streamed batch, built in ONE launch directly behind the streaming sampler (no new ABI number: callers detect
 * it by its symbol): step 1 of evaluation.sh, evaluation/compute_gt_pose.py:80-89 run with --nocs ANCSH and with --nocs NAOCS.  rows,
 * capacity, offsets (b + 1), perm (b, n) and nchan == 18 are what ancsh_point_gt_rec reads: sampled point i of cloud c is raw row
 * offsets[c] + perm[c][i] % n_raw; cls_gt = the C truncation of channel 3, nocs_p = channels 4..6, nocs_g = channels 7..9.  P (b, n, ldp >= 3)
 * float32: the sampled, scaled points the networks read (the P of the reference's prediction record).  extent: row (c, j) = the 3 float64
 * values at extent + (c * K + j) * ld_extent (a pipeline points it at column 13 of the submitted ground truth, ld_extent = 19); NULL = NaN.
 * gt (b, K, 19) and frame (b, 13) float64, out of place; either may be NULL to skip it.
 * For part j of cloud c, over the sampled points with cls_gt == j in sample order:
 *   U_p = estimateSimilarityUmeyama(nocs_p, P),  U_g = estimateSimilarityUmeyama(nocs_g, P)  (lib/aligning.py:580-622),
 * each THE BITS ancsh_umeyama writes for those rows gathered into a contiguous problem (one statement of the arithmetic, csrc/umeyama_fit.h:
 * float64, thread t of 256 takes compacted rows t, t + 256, ..., the same reductions in the same order).
 *   gt[c][j][0..8]   U_p's src -> tgt rotation, row-major: the transpose of ancsh_umeyama's Rotation, compose_rt's upper 3 x 3
 *   gt[c][j][9]      U_p's scale, float64 as computed        gt[c][j][10..12]  U_p's translation
 *   gt[c][j][13..15] the extent row, bit for bit (a NaN keeps its payload)      gt[c][j][16..18]  U_g's translation
 *   frame[c]         [R (9) | s | t (3)] of U_g for part 0
 * Every R and t entry is rounded to float32 once and widened: compose_rt's float32 matrix, what pack_ground_truth / pack_joint_frame
 * receive from the pickles.  These are the rows ancsh_gt_error_rec (gt) and ancsh_point_gt_rec (frame) read.
 * NaN rules.  A non-finite fit: a fit whose 13 numbers [R | s | t] contain a non-finite value gives NaN in all 13 (one point, coincident
 * NOCS -- varP == 0 --, a non-finite P); U_p's 13 are columns 0..12, of U_g's 13 the row holds 16..18 and the frame all.  An empty part:
 * if ANY part of the cloud has no sampled ground-truth point the whole cloud is missing -- columns 0..12 and 16..18 of all K rows are NaN
 * and so is the frame (the reference skips such a record, compute_gt_pose.py:98-99); cls_gt outside [0, K) belongs to no part.  Bad
 * offsets: a cloud whose rows are empty or reach outside [0, capacity) gets NaN throughout, extent columns included.  A cloud never
 * changes a neighbour's bytes.  K == 1 is legal.
 * One workgroup per (part, cloud); each counts all K parts, then compacts its part's samples in order into LDS (n <=
 * ANCSH_ARTICULATION_MAX_N).  Graph-capturable: every cloud size is read from device memory, nothing is allocated, no atomics, no
 * workgroup waits for another; the same bytes on every run and wherever the cloud lies in the batch.  b == 0 launches nothing.
 * Checked before any launch (-1, ancsh_last_error): 0 <= b <= 65535, 1 <= K <= 8, nchan == 18, 1 <= n <= 4096, ldp >= 3, ld_extent >= 3
 * when extent is set, 0 <= capacity < 2^30, null rows / offsets / perm / P, gt and frame both NULL. */
int ancsh_gt_pose_build(int b, int n, int K, int nchan, const float *rows, long capacity, const int *offsets, const int *perm,
                        const float *P, int ldp, const double *extent, int ld_extent, double *gt, double *frame, void *stream);

/* ---- input sampling in front of the network (lib/dataset.py:290-357) ------------------------ */

/* One launch for a ragged batch: cloud b owns raw rows [offsets[b], offsets[b+1]) of `rows` (nchan floats each:
 * x y z then per-point channels).  Sampled row i of cloud b = raw row perm[b*num_points+i] % n_raw (the reference's
 * tiling, :290-317, is this modulo), giving P (b,N,3) = xyz * norm_factor[b] (:346), chan_out (b,N,nchan-3) = the other
 * channels, mask_array (b,N,n_parts) = one-hot of int8(row[cls_col]) with numpy's negative-index rule (:357) and
 * joint_cls_mask (b,N) = row[jcls_col] > 0 (:353-355; jcls_col < 0: zeros). */
int ancsh_input_sample(int nclouds, int num_points, int nchan, const float *rows, const int *offsets, const int *perm,
                       const float *norm_factor, int cls_col, int jcls_col, int n_parts, float *P, float *chan_out,
                       float *mask_array, float *joint_cls_mask, void *stream);

/* The sampler of the streaming pipeline: one launch per batch in which every size-dependent value is read from DEVICE memory,
 * so one captured graph serves any cloud sizes up to `capacity` rows.  Cloud b owns raw rows [offsets[b], offsets[b+1]) of `rows`
 * (capacity x nchan float32: x y z, then channels; nchan >= 4).  With n_raw = offsets[b+1] - offsets[b] and N = num_points, the
 * reference's tiled size (lib/dataset.py:290-293) is T = n_raw if n_raw >= N else (N / n_raw + 1) * n_raw, and sampled row i of
 * cloud b is raw row pi_b(i) % n_raw, where pi_b is a keyed bijection of [0, T) -- so the N rows are N distinct rows of the tiled
 * cloud, as np.random.permutation(T)[:N] picks them (:341-351), without a sort, a scan or per-cloud host work:
 *   w  = the smallest even number with 2^w >= T, h = w / 2, mask = 2^h - 1;
 *   key[r] = splitmix64(s ^ splitmix64(0xF000000000000000 | b << 8 | r)), r = 0..3, s = *seed (uint64, device memory);
 *   F(x): L = x >> h, R = x & mask; four rounds of  (L, R) = (R, L ^ (splitmix64(key[r] ^ R) & mask)); F(x) = L << h | R;
 *   pi_b(i) = the first of F(i), F(F(i)), ... that is < T (cycle walking: 2^w < 4T, < 4 rounds of F on average).
 * splitmix64(x): x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^ x >> 31
 * (all mod 2^64; the pose generator's finaliser; the tag bits 60..63 keep the sampler's keys apart from its draw keys).
 * Outputs: P (nclouds, N, 3) = xyz * norm_factor[b] (:346); joint_cls (nclouds, N) int32 = the C truncation of channel jcls_col
 * (np.asarray(x, np.int32)); perm_out (nclouds, N) int32 = pi_b(i) (NULL: not written).  A cloud with n_raw == 0 or rows outside
 * [0, capacity) leaves its outputs untouched (callers refuse such clouds on the host).  Checked before any launch: nchan >= 4,
 * 3 <= jcls_col < nchan, 0 <= capacity < 2^30, nclouds <= 65535 (grid), null pointers (perm_out may be NULL). */
int ancsh_input_sample_stream(int nclouds, int num_points, int nchan, const float *rows, long capacity, const int *offsets,
                              const float *norm_factor, int jcls_col, const unsigned long long *seed, float *P, int *joint_cls,
                              int *perm_out, void *stream);

/* ancsh_input_sample_stream with the key block (ancsh_stream_key above) in place of the bare seed: the Feistel round keys use the
 * GLOBAL cloud index, key[r] = splitmix64(s ^ splitmix64(0xF000000000000000 | (cloud_base + b) << 8 | r)), s = key->seed.  So clouds
 * [lo, hi) sampled with cloud_base = lo give P, joint_cls and perm_out equal to rows [lo, hi) of the whole batch sampled with base 0,
 * and base 0 gives the bytes of ancsh_input_sample_stream.  Same checks; key == NULL is refused.  The kernel is the unkeyed one with a
 * template flag; the unkeyed instantiation is unchanged. */
int ancsh_input_sample_stream_keyed(int nclouds, int num_points, int nchan, const float *rows, long capacity, const int *offsets,
                                    const float *norm_factor, int jcls_col, const ancsh_stream_key *key, float *P, int *joint_cls,
                                    int *perm_out, void *stream);

/* The xyz-only twins of the two entries above (ABI 13): rows of nchan >= 3 channels, x y z first, no joint-class channel, no
 * joint_cls output.  P and perm_out are bit-equal to those of ancsh_input_sample_stream / _keyed on the same xyz, seed, key and
 * cloud_base (the permutation depends only on n_raw, the key and the cloud index).  The same kernel behind a template flag; the 4-column
 * instantiations are unchanged.  Checked before any launch: nchan >= 3, 0 <= capacity < 2^30, nclouds <= 65535, null seed / key, null
 * pointers (perm_out may be NULL). */
int ancsh_input_sample_stream_xyz(int nclouds, int num_points, int nchan, const float *rows, long capacity, const int *offsets,
                                  const float *norm_factor, const unsigned long long *seed, float *P, int *perm_out, void *stream);
int ancsh_input_sample_stream_xyz_keyed(int nclouds, int num_points, int nchan, const float *rows, long capacity, const int *offsets,
                                        const float *norm_factor, const ancsh_stream_key *key, float *P, int *perm_out, void *stream);

/* The depth front end of the streaming pipeline (tools/preprocess_data.py:259-298: a mask picks the pixels, projMat back-projects them
 * into camera space, cloud_cam_real): masked depth crops -> the packed rows and offsets the samplers above read, in at most TWO launches
 * in which every size-dependent value is read from DEVICE memory, so one captured graph serves any crop sizes.  The ABI version is
 * unchanged; callers detect the entry by its symbol.
 *   depth : pixel_capacity depth values, uint16 (depth_type = ANCSH_DEPTH_U16) or float32 (ANCSH_DEPTH_F32), 16-byte aligned;
 *   mask  : pixel_capacity bytes, 8-byte aligned, or NULL = every pixel of a crop;
 *   geom  : (nclouds, 5) int32 {start, h, w, row0, col0}: cloud b's h x w crop lies row-major at depth[start .. start + h*w) (any start, not
 *           a prefix sum: clouds may share pixels, e.g. the padding clouds of a short batch) and its pixel (0, 0) is pixel (row0, col0) of
 *           the full image;
 *   cam   : (nclouds, 7) float32 {A00, A01, A02, A10, A11, A12, depth_scale}.
 * Pixel (i, j) of the crop, depth d, is VALID when its mask byte is non-zero (or mask == NULL) and d != 0 (uint16) / d > 0 && d < +inf
 * (float32: NaN, Inf, zero and negative depths are dropped).  Its point, with row = (float)(row0 + i), col = (float)(col0 + j), in exactly
 * this f32 arithmetic (no contraction):
 *   z = (float)d * depth_scale;  x = z * fmaf(A01, row, fmaf(A00, col, A02));  y = z * fmaf(A11, row, fmaf(A10, col, A12)).
 * Outputs: counts (nclouds) int32 = valid pixels per cloud; offsets (nclouds + 1) int32, offsets[0] = 0, offsets[b+1] = offsets[b] +
 * max(counts[b], 1) (saturating at 2^31 - 1); rows (capacity, 3) float32: cloud b's valid pixels in the row-major order of its crop
 * (np.where(mask)) at rows [offsets[b], offsets[b] + counts[b]).  A cloud without a valid pixel -- or whose crop has h < 1, w < 1 or lies
 * outside [0, pixel_capacity), which callers refuse on the host -- gets ONE row of three NaNs and counts[b] = 0: the sampler then hands the
 * network a non-finite cloud, whose record alone is poisoned.  Rows at and beyond offsets[nclouds] or capacity are left untouched; the
 * sum of h*w over the clouds should not exceed capacity (a cloud whose rows would pass it is cut there and refused by the samplers).
 * Deterministic byte for byte: a count pass (block (x, b) counts chunk x of cloud b's crop into scratch[b * chunks + x]) and a scatter pass
 * (each block sums the counts in front of its chunk and writes its rows in pixel order); no atomics, no block waits for another.
 * scratch: nclouds * ANCSH_DEPTH_MAX_CHUNKS int32 of working memory.  Graph-capturable: the grid depends on (pixel_capacity, nclouds) only;
 * no host sync, no allocation.  nclouds == 0 launches nothing.  Checked before any launch: 0 <= nclouds <= 65535, depth_type,
 * 0 <= pixel_capacity < 2^30, capacity >= pixel_capacity, null pointers (mask may be NULL), the two alignments. */
#define ANCSH_DEPTH_U16 0
#define ANCSH_DEPTH_F32 1
#define ANCSH_DEPTH_MAX_CHUNKS 64
int ancsh_depth_unproject_stream(int nclouds, int depth_type, const void *depth, const unsigned char *mask, long pixel_capacity,
                                 const int *geom, const float *cam, float *rows, long capacity, int *offsets, int *counts, int *scratch,
                                 void *stream);

/* The inverse of the depth front end's compaction: the per-row labels / values of ancsh_raw_point_labels back on the pixel grid of the
 * crops ancsh_depth_unproject_stream read -- per cloud a label image and a 7-channel value image (the NOCS map), in ONE launch on the
 * depth entry's grid.  The ABI version is unchanged; callers detect the entry by its symbol.
 *   nclouds, depth_type, depth, mask, pixel_capacity, geom : exactly what the ancsh_depth_unproject_stream call was given;
 *   offsets (nclouds + 1), scratch : what that call WROTE (scratch holds the count pass's per-chunk counts: nothing may write it
 *           between the two calls);
 *   labels (capacity) int32, values (capacity, 7) float32 : per row, as ancsh_raw_point_labels writes them (nchan = 3);
 *   dest (nclouds) int32 : cloud b's image starts at element dest[b] of the image buffers; dest[b] < 0 silences the cloud (the padding
 *           clouds of a short batch alias another cloud's pixels but hold other labels);
 *   img_labels (image_capacity) int32, img_values (image_capacity, 7) float32 : the images.
 * For cloud b with crop h x w at `start` and dest[b] >= 0, pixel (i, j), q = dest[b] + i * w + j: the pixel is VALID by the depth entry's
 * rule; rank = the valid pixels in front of it in row-major order; r = offsets[b] + rank.  Valid and r < capacity: img_labels[q] =
 * labels[r] and img_values[q][0..6] = values[r][0..6], bit for bit (NaN payloads included).  Otherwise (background, hole, masked out, a
 * row cut at capacity): img_labels[q] = -1 and seven NaNs of the bit pattern ANCSH_LABEL_NAN_BITS, the one ancsh_raw_point_labels writes
 * with label -1.  Every pixel of the crop is written (no prefill needed); image elements of no cloud's crop are left untouched.  A cloud
 * with dest[b] < 0, with a crop the depth entry treats as empty (h < 1, w < 1, outside [0, pixel_capacity)), or with dest[b] + h * w >
 * image_capacity writes NOTHING.  Images of different clouds must not overlap (clouds may share source pixels).  Deterministic byte for
 * byte: no atomics, no block waits for another.  Graph-capturable: the grid depends on (pixel_capacity, nclouds) only, every size is read
 * from device memory; no host sync, no allocation.  nclouds == 0 launches nothing.  Checked before any launch: 0 <= nclouds <= 65535,
 * depth_type, 0 <= pixel_capacity < 2^30, 0 <= capacity, image_capacity < 2^30, null pointers (mask may be NULL), the two alignments
 * (depth 16 bytes, mask 8 bytes; the outputs need none beyond their element's). */
#define ANCSH_LABEL_NAN_BITS 0x7fc00000u
int ancsh_depth_label_images(int nclouds, int depth_type, const void *depth, const unsigned char *mask, long pixel_capacity,
                             const int *geom, const int *offsets, const int *scratch, const int *labels, const float *values,
                             long capacity, const int *dest, int *img_labels, float *img_values, long image_capacity, void *stream);

/* Rendered depth frames annotated on the device: the step of tools/preprocess_data.py:259-320 that makes a frame's gt_points and gt_coords,
 * and the order in which lib/dataset.py:475-485 concatenates them -- depth crops, link-label crops and one scene table per frame -> the
 * 7-column rows [x y z | cx cy cz | part] ancsh_point_gt_build reads (dataset.pack_annotated_cloud's), in TWO launches on
 * ancsh_depth_unproject_stream's grid and chunking.  The ABI version is unchanged; callers detect the entry by its symbol.
 *   nclouds, depth_type, depth, pixel_capacity, geom : as ancsh_depth_unproject_stream takes them;
 *   labels : pixel_capacity bytes, 8-byte aligned (never NULL): a pixel's byte is its link index; 255, or any value >= nlinks, is not object;
 *   scene  : (nclouds, ANCSH_SCENE_WIDTH = 240) float64, 8-byte aligned, per cloud:
 *     [0..5] A00 A01 A02 A10 A11 A12 of gt_points (cloud_cam_real, :293-296, v1 = row * 2 / H - 1)   [6] depth_scale
 *     [7..12] C00 C01 C02 C10 C11 C12 of the coordinate point (cloud_cam, :288-291, v = (H - row) * 2 / H - 1)
 *     [13] min_link_pixels (:279-281: 10)   [14] nlinks, 1..ANCSH_SCENE_MAX_LINKS   [15] reserved, 0
 *     then per link l, ANCSH_SCENE_LINK = 14 wide, at ANCSH_SCENE_HEAD + 14 l:  [0] rank = the link's position in the flattened
 *     parts_map, -1 = the link is not used (its pixels are dropped and it does not count for the minimum)   [1] part = its group's index
 *     [2..13] M, row-major 3 x 4: camera -> URDF frame of the link, the chain of :298-320 composed on the host in float64
 *     (pinv(viewMat.T) with its first three rows negated, pinv(parts_model2world[l].T), my_canon2urdf_mat.T).
 * Pixel (i, j) of the crop, label l, depth d, is VALID when l names a used link and d != 0 (uint16) / d > 0 && d < +inf (float32) -- the
 * rule of ancsh_depth_unproject_stream.  (The reference keeps every labelled pixel, holes included: its renderer leaves none on an object.)
 * Its row, with row = row0 + i, col = col0 + j as float64, in exactly this float64 arithmetic (no contraction), every output rounded to
 * float32 once:
 *   z = d * depth_scale;  x = z * ((A00 col + A01 row) + A02);  y = z * ((A10 col + A11 row) + A12);
 *   x' = z * ((C00 col + C01 row) + C02);  y' = z * ((C10 col + C11 row) + C12);
 *   c_a = ((M[a][0] x' + M[a][1] y') + M[a][2] z) + M[a][3], a = 0..2;   the row is [x y z | c_0 c_1 c_2 | part].
 * A cloud in which a used link has fewer than min_link_pixels valid pixels has no rows (the reference skips such a frame); otherwise its
 * rows are its valid pixels sorted by (rank of the link, row-major pixel order): a stable counting sort, so the rows of a part are
 * neighbours, in the order lib/dataset.py:475-485 gives them.
 * Outputs: link_counts (nclouds, 16) int32 = valid pixels per link (0 for a link that is not used), whether or not the cloud passes the
 * minimum; counts (nclouds) int32 = rows per cloud; offsets (nclouds + 1) int32, offsets[0] = 0, offsets[b+1] = offsets[b] + max(counts[b],
 * 1) (saturating at 2^31 - 1); rows (capacity, 7) float32.  A cloud without rows -- or whose crop has h < 1, w < 1 or lies outside [0,
 * pixel_capacity), or whose scene's nlinks is outside 1..16 -- gets ONE row of seven NaNs and counts[b] = 0: ancsh_point_gt_build makes
 * an all-NaN row of it, and the cloud's record alone is poisoned.  Rows at and beyond offsets[nclouds] or capacity are left untouched.
 * Deterministic byte for byte: a count pass (block (x, b) writes the 16-entry histogram of chunk x of cloud b into scratch[(b * chunks + x) *
 * 16 ..]) and a scatter pass (each block derives every start it needs from the histograms and ranks its pixels with per-link wave
 * ballots); no atomics, no block waits for another.  scratch: nclouds * ANCSH_DEPTH_MAX_CHUNKS * 16 int32 of working memory.
 * Graph-capturable: the grid depends on (pixel_capacity, nclouds) only; no host sync, no allocation.  nclouds == 0 launches nothing.
 * Checked before any launch: 0 <= nclouds <= 65535, depth_type, 0 <= pixel_capacity < 2^30, pixel_capacity <= capacity < 2^30, null
 * pointers, the three alignments (depth 16 bytes, labels and scene 8 bytes). */
#define ANCSH_SCENE_WIDTH 240
#define ANCSH_SCENE_MAX_LINKS 16
#define ANCSH_SCENE_HEAD 16
#define ANCSH_SCENE_LINK 14
int ancsh_depth_annotate_stream(int nclouds, int depth_type, const void *depth, const unsigned char *labels, long pixel_capacity,
                                const int *geom, const double *scene, float *rows, long capacity, int *offsets, int *counts,
                                int *link_counts, int *scratch, void *stream);

/* The inverse of that entry's stable counting sort: what lies per ROW of an annotated frame -- the networks' label and values
 * (ancsh_raw_point_labels over the 18-column rows, nchan = 18) and the ground truth of those rows (ancsh_point_gt_build) -- back on the
 * pixel grid of the crops ancsh_depth_annotate_stream read: per cloud a predicted part image and 7-channel value image, and the true part
 * image and 6-channel NOCS image, in ONE launch on the depth entries' grid and chunking.  The ABI version is unchanged; callers detect the
 * entry by its symbol.
 *   nclouds, depth_type, depth, link_labels, pixel_capacity, geom, scene : exactly what the ancsh_depth_annotate_stream call was given;
 *   offsets (nclouds + 1), counts (nclouds), scratch : what that call WROTE (scratch holds the count pass's per-chunk histograms: nothing
 *           may write it between the two calls);
 *   labels (capacity) int32, values (capacity, 7) float32 : per row, as ancsh_raw_point_labels writes them;
 *   gt_rows (capacity, gt_nchan) float32 : the rows of ancsh_point_gt_build (gt_nchan = 18): column 3 the part, 4..6 the part NOCS, 7..9
 *           the NAOCS;
 *   dest (nclouds) int32 : cloud b's images start at element dest[b] of the image buffers; dest[b] < 0 silences the cloud (the padding
 *           clouds of a short batch alias another cloud's pixels);
 *   img_labels (image_capacity) int32, img_values (image_capacity, 7) float32 : the predicted images;
 *   img_gt_labels (image_capacity) int32, img_gt_values (image_capacity, 6) float32 : the true ones.
 * For cloud b with crop h x w and dest[b] >= 0, pixel (i, j), q = dest[b] + i * w + j: the pixel is VALID by the annotate entry's rule (its
 * label names a used link and its depth passes) and, in addition, counts[b] > 0 -- a cloud in which a used link is below the scene's
 * minimum has no rows, and all its pixels read background.  The row of a valid pixel is the one the scatter pass gave it: r = offsets[b] +
 * the cloud's totals of the links of smaller rank + the valid pixels of its own link in front of it in row-major order.  Valid and r <
 * capacity, bit for bit (NaN payloads included): img_labels[q] = labels[r]; img_values[q][0..6] = values[r][0..6]; img_gt_labels[q] =
 * (int)gt_rows[r][3], or -1 when that value is not finite; img_gt_values[q][0..5] = gt_rows[r][4..9].  Otherwise (background, hole, a
 * link that is not used, a cloud without rows, a row cut at capacity): both labels -1 and every value channel NaN of the bit pattern
 * ANCSH_LABEL_NAN_BITS.  Every pixel of the crop is written (no prefill needed); image elements of no cloud's crop are left untouched.  A
 * cloud with dest[b] < 0, with a crop the annotate entry treats as empty (h < 1, w < 1, outside [0, pixel_capacity)), or with dest[b] + h *
 * w > image_capacity writes NOTHING.  Images of different clouds must not overlap (clouds may share source pixels).  Deterministic byte
 * for byte: each block derives its links' first rows from its own cloud's histograms and ranks its pixels with per-link wave ballots, as
 * the scatter pass does; no atomics, no block waits for another.  Graph-capturable: the grid depends on (pixel_capacity, nclouds) only,
 * every size is read from device memory; no host sync, no allocation.  nclouds == 0 launches nothing.  Checked before any launch: 0 <=
 * nclouds <= 65535, depth_type, 0 <= pixel_capacity < 2^30, 0 <= capacity < 2^30 (the rows are only read: a capacity below the annotate
 * call's cuts the rows at and beyond it), gt_nchan >= 10, 0 <= image_capacity < 2^30, null pointers, the annotate entry's three alignments
 * (depth 16 bytes, link_labels and scene 8 bytes; the outputs need none beyond their element's). */
int ancsh_depth_annotated_images(int nclouds, int depth_type, const void *depth, const unsigned char *link_labels, long pixel_capacity,
                                 const int *geom, const double *scene, const int *offsets, const int *counts, const int *scratch,
                                 const int *labels, const float *values, const float *gt_rows, int gt_nchan, long capacity,
                                 const int *dest, int *img_labels, float *img_values, int *img_gt_labels, float *img_gt_values,
                                 long image_capacity, void *stream);

/* Depth and link-label frames of an articulated object rendered on the device: triangle meshes, one render table per frame and the depth
 * entries' geometry rows -> depth crops and label crops in exactly the buffers ancsh_depth_annotate_stream reads.  The reference renders
 * on the host, one frame at a time (tools/render_synthetic.py:180-225, pybullet's getCameraImage); pixel parity with that rasteriser is no
 * goal.  The contract is geometric: this entry is the exact inverse of the camera model ancsh_depth_annotate_stream applies to a frame's
 * coordinate point (scene[7..12], the C coefficients).  The ABI version is unchanged; callers detect the entry by its symbol.
 *   nframes, depth_type, geom, pixel_capacity : as the depth entries take them; geom (nframes, 5) int32 {start h w row0 col0} names the crop
 *     to render and where it lies in the pixel buffers;
 *   verts (V, 3) float32 : every link's vertices in its model frame (the frame the link's world pose places; the URDF visual origin is the
 *     caller's to apply);  tris (T, 3) int32 : vertex indices;  tri_link (T,) int32 : the link of a triangle, in [0, 16);
 *   render : (nframes, ANCSH_RENDER_WIDTH = 208) float64, 8-byte aligned, per frame:
 *     [0..5] P00 P01 P02 P10 P11 P12 : col = (P00 s + P01 t) + P02, row = (P10 s + P11 t) + P12 -- the inverse of the affine map
 *     s = C00 col + C01 row + C02, t = C10 col + C11 row + C12 of scene[7..12]   [6] depth_scale   [7] z_min > 0   [8] nlinks, 1..16
 *     [9] reserved, 0 (the *_lib entries: the frame's instance)   [10..15] reserved, 0   then per link l, ANCSH_RENDER_LINK = 12 wide, at ANCSH_RENDER_HEAD + 12 l: R, row-major 3 x 4, model frame ->
 *     the camera point (x', y', z);
 *   depth (pixel_capacity) of depth_type, 16-byte aligned; labels (pixel_capacity) bytes, 8-byte aligned; zbuf (pixel_capacity) uint64 of
 *     working memory, 8-byte aligned.
 * Everything below is float64, evaluated in exactly the written order (no contraction).
 *   Vertex v of link l: q_a = ((R[a][0] v0 + R[a][1] v1) + R[a][2] v2) + R[a][3];  z = q_2, s = q_0 / z, t = q_1 / z;  col, row as above;
 *   fixed point X = rint(256 col), Y = rint(256 row) (int64).  A triangle is dropped WHOLE (no clipping: the reference's camera stands off
 *   the object) when a vertex has z < z_min, a non-finite value, |X| or |Y| >= 2^25, an index outside [0, V), or when its link is
 *   outside [0, nlinks).
 *   The sample point of crop pixel (i, j) is full-image (row0 + i, col0 + j) exactly, no half-pixel offset -- the point
 *   ancsh_depth_annotate_stream unprojects --: p = (256 (col0 + j), 256 (row0 + i)) in (X, Y).
 *   Coverage, int64: E_uv(p) = (v.X - u.X)(p.Y - u.Y) - (v.Y - u.Y)(p.X - u.X); for the triangle (a, b, c): area2 = E_ab(c) (zero: the
 *   triangle is dropped; both orientations are kept, no back-face culling), E_a = E_bc(p), E_b = E_ca(p), E_c = E_ab(p); p is covered
 *   when E_a, E_b, E_c all have the sign of area2 or are zero.
 *   Depth, perspective-correct: lambda_k = (double)E_k / (double)area2 (both exact: below 2^53);
 *   invz = (lambda_a (1 / z_a) + lambda_b (1 / z_b)) + lambda_c (1 / z_c);  d = 1 / invz.
 *   The pixel keeps the MINIMUM key (bits of (float)d) << 32 | triangle index over the triangles that cover it: the nearest surface, ties
 *   to the lowest triangle index.  A minimum does not depend on the order: the result is deterministic byte for byte.
 *   Resolve, df = (double)(float)d: uint16: q = rint(df / depth_scale), written when 1 <= q <= 65535; float32: (float)(df / depth_scale),
 *   written when finite and positive; labels = tri_link[winner].  Every other pixel of the crop reads depth 0 and label 255.  EVERY pixel
 *   of every crop is written (no prefill needed); pixels of no crop are left alone.
 * A frame whose nlinks is outside 1..16 or whose z_min is not > 0 renders an all-background crop; a frame with h < 1 or w < 1 or whose
 * crop lies outside [0, pixel_capacity) writes nothing.  Crops that share pixels (the padding frames of a short batch alias the first
 * frame's) must carry the same table: each launch finishes before the next starts, so equal frames write equal bytes.
 * Three launches: clear (the keys of every crop), raster (one wave per (triangle, frame): the wave sweeps the triangle's bounding box clipped
 * to the crop, one 64-bit integer atomic minimum per covered pixel), resolve.  Graph-capturable: the grids depend on (pixel_capacity,
 * nframes, T) only; no host sync, no allocation.  nframes == 0 launches nothing and returns 0; T == 0 renders background.
 * Checked before any launch: 0 <= nframes <= 65535, depth_type, 0 <= pixel_capacity < 2^30, 0 <= T < 2^24, 0 <= V < 2^24, null pointers,
 * the alignments (depth 16 bytes; labels, render, zbuf 8 bytes). */
#define ANCSH_RENDER_WIDTH 208
#define ANCSH_RENDER_HEAD 16
#define ANCSH_RENDER_LINK 12
int ancsh_render_depth_labels(int nframes, int depth_type, const float *verts, const int *tris, const int *tri_link, int V, int T,
                              const int *geom, const double *render, void *depth, unsigned char *labels, unsigned long long *zbuf,
                              long pixel_capacity, void *stream);

/* Both tables of a rendered, annotated frame built on the device: an object's kinematic table and one pose per frame (joint values and a
 * view matrix) -> the render table ancsh_render_depth_labels reads and the scene table ancsh_depth_annotate_stream reads, in exactly their
 * layouts.  The reference takes the link poses from pybullet's forward kinematics on the host (tools/render_synthetic.py:140-158, 206-217),
 * and depth.pack_render_scene / depth.pack_frame_scene compose every link's maps with pinv / inv on 4 x 4 matrices, one frame at a time; for
 * rigid matrices both reduce to the closed forms below, which need no inverse.  The reference rounds the link poses it stores to float32
 * (tools/preprocess_data.py:235-236, an artefact of its YAML files): poses here are float64 throughout.  The ABI version is unchanged;
 * callers detect the entry by its symbol.
 *   kin  : one table per object, ANCSH_KIN_WIDTH = 672 float64 (ANCSH_KIN_HEAD = 32, then 16 links x ANCSH_KIN_LINK = 40), 8-byte aligned:
 *     head [0..15] the scene table's head, verbatim (A coefficients, depth_scale, C coefficients, min_link_pixels, nlinks, 0)
 *          [16..21] the render table's pixel map P00 P01 P02 P10 P11 P12   [22] z_min   [23..31] reserved, 0
 *     link l at 32 + 40 l:  [0] rank  [1] part (as in the scene table)   [2] parent: -1 for link 0, the only root, otherwise < l
 *          [3] joint kind: 0 fixed, 1 revolute, 2 prismatic   [4..15] T_l, row-major 3 x 4: the URDF joint origin Rz(yaw) Ry(pitch) Rx(roll)
 *          | xyz, from the parent link's frame to link l's frame at q = 0 (link 0: its world pose; the reference's is the identity)
 *          [16..18] the unit joint axis a in link l's frame   [19..27] Rc_l, row-major 3 x 3, and [28..30] offset_l: the rotation and the
 *          offset of the link's canon2urdf map (depth.pack_frame_scene's)   [31..39] reserved, 0
 *   pose : (nframes, ANCSH_POSE_WIDTH = 32) float64, 8-byte aligned, per frame:
 *     [0..15] q_l, link l's joint value in radians (revolute) or length units (prismatic); ignored for link 0 and for fixed joints
 *     [16..27] V, the first three rows of the view matrix (world -> eye, the `.reshape(4, 4).T` form of tools/preprocess_data.py:228),
 *     row-major 3 x 4; it must be rigid (the host checks it)   [28] reserved, 0 (ancsh_pose_scene_build_lib: the frame's instance)
 *     [29..31] reserved, 0
 *   render (nframes, ANCSH_RENDER_WIDTH) and scene (nframes, ANCSH_SCENE_WIDTH) float64, 8-byte aligned: the outputs; every value of every
 *     frame's tables is written.
 * Everything below is float64, evaluated in exactly the written order (no contraction); (s, c) = sincos(q) are the only values that are not
 * a fixed sequence of IEEE operations, and sincos(0) = (0, 1) exactly.  A 3 x 4 map [R | t] stands for the rigid 4 x 4 matrix.
 *   Composition C = A o B:  C[i][j] = (A[i][0] B[0][j] + A[i][1] B[1][j]) + A[i][2] B[2][j], for j = 3 then + A[i][3].
 *   Joint motion J_l(q) = [Rj | tj]; fixed joints and link 0: [I | 0]; prismatic: [I | (q a_0, q a_1, q a_2)]; revolute: tj = 0 and
 *     Rj[i][j] = (c d_ij + s K[i][j]) + ((1 - c) a_i) a_j with d the identity and K = [a]x = {0 -a2 a1; a2 0 -a0; -a1 a0 0}.
 *   X_l = T_l o J_l (always composed, the identity included).
 *   World pose, from the leaf upwards: W = X_l, then for p = parent(l), parent(p), ..., 0: W <- X_p o W.
 *   A_l = V o W = [Ra | ta].  The render map of link l is R_l = -A_l, entry by entry.
 *   The scene map of link l:  M[i][j] = -((Rc[i][0] Ra[j][0] + Rc[i][1] Ra[j][1]) + Rc[i][2] Ra[j][2]) for j = 0..2, and
 *     M[i][3] = ((M[i][0] ta_0 + M[i][1] ta_1) + M[i][2] ta_2) + offset_i;  rank and part are copied from kin.
 *   Heads, copied bit for bit: scene[0..15] = kin[0..15]; render[0..5] = kin[16..21], render[6] = kin[6], render[7] = kin[22],
 *     render[8] = kin[14], render[9..15] = 0.  Links >= nlinks (nlinks outside 1..16: every link) read 0 in both tables.
 * M_l (R_l (v, 1), 1) = Rc_l v + offset_l: the two maps are each other's inverse up to the link's canon2urdf map, which is what
 * depth.pack_render_scene and depth.pack_frame_scene give for the same link poses.
 * One launch, one thread per (frame, link), the grid a function of nframes alone; no host sync, no allocation: graph-capturable.  A few
 * thousand double multiply-adds per frame: the launch sits on the floor of a dependent graph node.  nframes == 0 launches nothing and
 * returns 0.  Checked before any launch: 0 <= nframes <= 65535, null pointers, the 8-byte alignments. */
#define ANCSH_KIN_WIDTH 672
#define ANCSH_KIN_HEAD 32
#define ANCSH_KIN_LINK 40
#define ANCSH_POSE_WIDTH 32
int ancsh_pose_scene_build(int nframes, const double *kin, const double *pose, double *render, double *scene, void *stream);

/* Crops centred on the projected object: for every frame whose geometry row holds ANCSH_CROP_CENTRE (INT32_MIN; a real origin lies below
 * 2^24 in magnitude) in BOTH row0 and col0, the origin that centres the h x w crop on the bounding box of the object's projected vertices is
 * written into the row; every other frame is left alone, so a second call -- a replay that finds real origins -- is a no-op.
 *   verts, tris, tri_link, V, T, render : as ancsh_render_depth_labels takes them;  geom (nframes, 5) int32 {start h w row0 col0}: read and,
 *     for centred frames, row0 and col0 written (start, h, w are untouched);  bounds (nframes, 4) int32 of working memory, initialised here.
 * A vertex COUNTS when a triangle whose link is in [0, nlinks) references it, its index is in [0, V), and ancsh_render_depth_labels' vertex
 * transform (the same device function: z, X = rint(256 col), Y = rint(256 row)) keeps it: every value finite, z >= z_min, |X|, |Y| < 2^25.
 * Vertices count one by one, not per dropped triangle.  With Xmin, Xmax, Ymin, Ymax over the counted vertices (int32):
 *   col0 = ((Xmin + Xmax) >> 9) - (w >> 1),  row0 = ((Ymin + Ymax) >> 9) - (h >> 1)   (arithmetic shifts: floor);
 * a frame without a counted vertex (T == 0, nlinks outside 1..16, everything behind z_min) gets (0, 0).
 * One launch, one block per frame (the grid depends on nframes alone): a wave reduces its vertices' bounds with shuffles and takes one int32
 * atomicMin / atomicMax per bound on the frame's row of `bounds`; minimum and maximum do not depend on the order of their operands, so the
 * origins are a pure function of the input.  The padding frames of a short batch carry the first frame's table and crop, so they write the
 * same origin.  Graph-capturable: no host sync, no allocation.  nframes == 0 launches nothing and returns 0.  Checked before any launch:
 * 0 <= nframes <= 65535, 0 <= T < 2^24, 0 <= V < 2^24, null pointers, the alignments (render 8 bytes; geom, bounds 4 bytes). */
#define ANCSH_CROP_CENTRE (-2147483647 - 1)
int ancsh_render_centre_crops(int nframes, const float *verts, const int *tris, const int *tri_link, int V, int T, const double *render,
                              int *geom, int *bounds, void *stream);

/* A LIBRARY of object instances behind the three entries above: many meshes and many kinematic tables uploaded once, and the instance of a
 * frame chosen on the device from a reserved value of the table that already travels per frame -- pose[28] for ancsh_pose_scene_build_lib,
 * render[9] (which that entry writes) for the two others.  The single-object entries keep their contracts: they read neither value.  The
 * reference renders one instance after the other on the host (tools/render_synthetic.py:52, one render_data call per name_obj).  The ABI
 * version is unchanged; callers detect the entries by their symbols.
 *   The library: the instances' meshes concatenated -- verts (V, 3) float32, tris (T, 3) int32 whose indices are GLOBAL (each instance's
 *   vertex base already added), tri_link (T,) int32 -- and tri_off (ninst + 1,) int32, non-decreasing, tri_off[0] = 0, tri_off[ninst] = T:
 *   instance i owns triangles [tri_off[i], tri_off[i + 1]).  kin (ninst, ANCSH_KIN_WIDTH) float64: instance i's table at kin + 672 i.
 *   1 <= ninst <= ANCSH_LIBRARY_MAX_INSTANCES; V, T < 2^24 as before (the z-buffer key keeps the GLOBAL triangle index in its low word).
 *   The instance of a frame: i = the value when it is an integer in [0, ninst); any other value (NaN fails every comparison) makes the
 *   table "not one", as a bad nlinks does.  So do offsets tri_off[i], tri_off[i + 1] that are no range inside [0, T].
 * ancsh_render_depth_labels_lib: ancsh_render_depth_labels in which frame f draws the triangles of instance render[f][9] only.  The same three
 *   launches; the raster grid is (ceil(Tmax / 4), nframes): the wave for LOCAL triangle j of frame f handles global triangle tri_off[i] + j
 *   and returns when that is >= tri_off[i + 1] (f is the block's y index: the lookup, two offsets per wave, is uniform over the wave, and
 *   nothing is read per pixel).  Tmax is an ARGUMENT: max_i (tri_off[i + 1] - tri_off[i]), computed by the caller from its host copy of
 *   tri_off and checked here to lie in [0, T]; no device value is read before the launches, so the grids depend on (pixel_capacity, nframes,
 *   Tmax) only and the entry stays graph-capturable.  A Tmax below the true maximum leaves the triangles past it undrawn.  Keys, ties (the
 *   lowest triangle index: global order within an instance is local order shifted) and the resolve step are unchanged, so a frame has, byte
 *   for byte, the depth and labels ancsh_render_depth_labels gives for that instance's own mesh.  A frame without an instance renders an
 *   all-background crop.  A library with very unequal instances launches idle waves for the small ones: they exit on the range test.
 * ancsh_render_centre_crops_lib: ancsh_render_centre_crops in which the block of a centred frame strides over its instance's triangles
 *   only; a frame without an instance counts no vertex and gets (0, 0).
 * ancsh_pose_scene_build_lib: frame f reads the table kin + 672 i, i = pose[f][28], and writes exactly what ancsh_pose_scene_build writes
 *   for that table (the same device function, sincos included) except render[9] = (double)i.  A frame without an instance gets both
 *   tables all zero: nlinks = 0, so the renderer writes background, the annotation counts 0 pixels and the record is all-NaN -- the path
 *   of a frame the reference skips.
 * Checked before any launch: what the single-object entry checks, 1 <= ninst <= 4096, tri_off non-null and 4-byte aligned, 0 <= Tmax <= T. */
#define ANCSH_LIBRARY_MAX_INSTANCES 4096
int ancsh_render_depth_labels_lib(int nframes, int depth_type, const float *verts, const int *tris, const int *tri_link, int V, int T,
                                  const int *tri_off, int ninst, int Tmax, const int *geom, const double *render, void *depth,
                                  unsigned char *labels, unsigned long long *zbuf, long pixel_capacity, void *stream);
int ancsh_render_centre_crops_lib(int nframes, const float *verts, const int *tris, const int *tri_link, int V, int T, const int *tri_off,
                                  int ninst, const double *render, int *geom, int *bounds, void *stream);
int ancsh_pose_scene_build_lib(int nframes, const double *kin, int ninst, const double *pose, double *render, double *scene, void *stream);

/* A depth sensor's defects applied to the frames above: range-dependent noise, holes, dropout at depth discontinuities and disparity
 * quantisation -- the clean depth and link-label crops ancsh_render_depth_labels writes (or a caller submits) -> degraded crops in a SECOND
 * pair of pixel buffers, which ancsh_depth_annotate_stream and ancsh_depth_annotated_images then read.  The reference has nothing here
 * (pybullet's depth is clean).  The annotation computes a pixel's canonical coordinates from the depth it is given, so a displaced point gets
 * the coordinates of the displaced point: per part the relation between camera point and NOCS stays an exact similarity, and the
 * ground-truth poses of ancsh_gt_pose_build are unchanged in exact arithmetic.  The ABI version is unchanged; callers detect the entries
 * by their symbols.
 *   nframes, depth_type, pixel_capacity, geom : as the depth entries take them; geom (nframes, 5) int32 {start h w row0 col0};
 *   depth_in, labels_in : the clean pixel buffers (pixel_capacity values of depth_type, 16-byte aligned; pixel_capacity bytes, 8-byte
 *     aligned); depth_out, labels_out : the degraded ones, same sizes and alignments.  No input range may overlap an output range, nor the
 *     two outputs each other (a pixel's neighbours are read from the clean input while other pixels are written): refused;
 *   scene : (nframes, ANCSH_SCENE_WIDTH) float64, 8-byte aligned; only value 6, depth_scale, is read;
 *   sensor : ONE table of ANCSH_SENSOR_WIDTH = 16 float64 for the launch, 8-byte aligned:
 *     [0..3] a0 a1 a2 z0 : sigma(z) = (a0 + a1 dz) + a2 (dz dz), dz = z - z0   [4] p_hole, in [0, 1]   [5] p_edge, in [0, 1]
 *     [6] edge_rel >= 0   [7] qd >= 0: focal length x baseline, in length units x pixels; 0 = no quantisation   [8] steps >= 1: disparity
 *     steps per pixel   [9] z_near   [10] z_far (may be +Inf)   [11..15] reserved, 0;
 *   seed : the device seed, 8-byte aligned (the _keyed entry: the key block, ancsh_stream_key).
 * Everything below is float64, evaluated in exactly the written order (no contraction).  No transcendental function appears: the result is
 * a fixed sequence of IEEE operations, byte-reproducible on the host.  Per crop pixel (i, j) of frame f, p = i w + j, g = base + f (base =
 * key->cloud_base; 0 for the seed entry), s the seed:
 *   1. The pixel is a SURFACE pixel when its label is not 255 and its stored depth is usable (uint16: >= 1; float32: finite and > 0).  Any
 *      other pixel is copied verbatim, depth and label.
 *   2. z = (double)stored * depth_scale.  The pixel is dropped unless z_near <= z && z <= z_far.
 *   3. Draws: r_k = splitmix64(s ^ splitmix64(0xE000000000000000 | g << 36 | p << 4 | k)), u_k = (double)(r_k >> 11) * 2^-53, splitmix64 the
 *      pose fit's generator.  The tag 0xE keeps these keys apart from the sampler's (0xF) and the draw keys' (0x0); the streams' bound
 *      (base + B) K < 2^20 keeps g below 2^20, and p < 2^30.
 *   4. Hole: dropped when u_0 < p_hole.
 *   5. Edge, evaluated only when p_edge > 0: the pixel is an edge pixel when any of its four neighbours INSIDE the crop is not a surface
 *      pixel or has |z_n - z| > edge_rel * z, z_n the neighbour's CLEAN depth from depth_in.  Neighbours outside the crop do not count.  An
 *      edge pixel is dropped when u_1 < p_edge.
 *   6. Noise: a, b = r_2 >> 32, r_2 & 0xFFFFFFFF and c, d likewise from r_3; S = a + b + c + d as an integer;
 *      n = ((double)S * 2^-32 - 2.0) * 1.7320508075688772 (Irwin-Hall of four, unit variance);  z1 = z + sigma(z) * n.
 *   7. Quantisation, when qd > 0: dq = rint((qd / z1) * steps) / steps; the pixel is dropped when !(dq > 0), otherwise z2 = qd / dq.  With
 *      qd = 0, z2 = z1.
 *   8. Store: when z2 has the bits of z the stored input value is copied verbatim; otherwise uint16 writes q = rint(z2 / depth_scale) when
 *      1 <= q <= 65535 and float32 writes (float)(z2 / depth_scale) when that is finite and positive, else the pixel is dropped.  The label
 *      is kept.
 * A dropped pixel reads depth 0 and label 255.  Two consequences: the all-zero table with z_far = +Inf is the IDENTITY, byte for byte; and
 * frames [lo, hi) run with cloud_base = lo give the bytes of rows [lo, hi) of the whole batch run with base 0.
 * EVERY pixel of every crop is written (no prefill needed); pixels of no crop are left alone.  A frame with h < 1, w < 1 or a crop outside
 * [0, pixel_capacity) writes nothing.  Crops that share pixels are written once per frame, with that frame's draws: give the frames of a
 * launch crops of their own.  One launch on the depth entries' grid and chunking, a function of (pixel_capacity, nframes) only; no atomics,
 * no host sync, no allocation: graph-capturable.  nframes == 0 launches nothing and returns 0.  Checked before any launch: 0 <= nframes <=
 * 65535, depth_type, 0 <= pixel_capacity < 2^30, null pointers, the alignments, the overlaps. */
#define ANCSH_SENSOR_WIDTH 16
int ancsh_depth_sensor_model(int nframes, int depth_type, const void *depth_in, const unsigned char *labels_in, long pixel_capacity,
                             const int *geom, const double *scene, const double *sensor, const unsigned long long *seed, void *depth_out,
                             unsigned char *labels_out, void *stream);
int ancsh_depth_sensor_model_keyed(int nframes, int depth_type, const void *depth_in, const unsigned char *labels_in, long pixel_capacity,
                                   const int *geom, const double *scene, const double *sensor, const ancsh_stream_key *key, void *depth_out,
                                   unsigned char *labels_out, void *stream);

/* Render-and-compare of a pose record, two entries around the unchanged renderer (no new ABI number: callers detect them by their symbols).
 * The object's own mesh is put where the fitted per-part poses say, rendered through the frame's camera by ancsh_render_depth_labels[_lib]
 * as 2 * nframes frames, and the predicted pixels are scored against the frame the annotation read: the check of a pose that needs no
 * ground truth.
 *
 * ancsh_reproject_scene_build: the map from a pose record back to render tables, ONE launch.
 *   render (nframes, ANCSH_RENDER_WIDTH), scene (nframes, ANCSH_SCENE_WIDTH) : the frame's own tables, as the renderer and the annotation read
 *     them;  rig (nframes, rig_ld = ANCSH_RIG_WIDTH(K)) : as ancsh_point_gt_build reads it;  norm_factor (nframes) float32 : the sampler's;
 *   record (nframes, K, ld) float64, ld >= 26 : columns 0..12 of row (f, j) are part j's baseline pose [R (9) row-major | s | t (3)], columns
 *     13..25 its nonlinear pose; the other columns are not read;
 *   geom (nframes, 5) int32 {start h w row0 col0} : the frame's geometry rows in a pixel buffer of pixel_capacity pixels;
 *   render_out (2 * nframes, ANCSH_RENDER_WIDTH) float64, geom_out (2 * nframes, 5) int32 : row v * nframes + f is frame f under variant v
 *     (0: the baseline pose, 1: the nonlinear pose), for a renderer call with 2 * nframes frames and 2 * pixel_capacity pixels.
 *   Heads: render_out[row][0..15] = render[f][0..15] bit for bit, the instance value [9] included.  geom_out[row] = geom[f] with start + v *
 *   pixel_capacity (a negative start is copied as it is; the sum saturates at 2^31 - 1): variant v draws into the v-th half of the buffers.
 *   Link l < nlinks (scene[14]) of part j = (int)scene link value [1], everything float64, evaluated in exactly the written order (no
 *   contraction), C = A o B being ancsh_pose_scene_build's composition of 3 x 4 maps:
 *     1. N = M_l o R_l : the frame's scene map composed with its render map, model frame -> canonical coordinates (= [Rc_l | offset_l] of
 *        ancsh_pose_scene_build up to rounding; composing the two tables makes the entry work without a kinematic table);
 *     2. Q, canonical coordinates -> part NOCS, ancsh_point_gt_build's nocs_p as a map: with sub, corner, factor, tail = part j's rig values
 *        [0..2], [3..5], [6..8], [9..11]:  o_a = ((((0 - sub_a) - corner_a) * factor_a) + 0.5) - tail_a;  rig[3] == 0: Q[a][k] = factor_k for
 *        a == k, else 0, Q[a][3] = o_a;  rig[3] != 0, with Rr = rig[4..12]: Q[a][k] = Rr[a][k] * factor_k,
 *        Q[a][3] = ((Rr[a][0] (o_0 - 0.5) + Rr[a][1] (o_1 - 0.5)) + Rr[a][2] (o_2 - 0.5)) + 0.5;
 *     3. P, part NOCS -> the scaled cloud, the record's pose of variant v: P[a][k] = s * R[a][k], P[a][3] = t_a;
 *     T1 = Q o N;  T2 = P o T1;
 *     4., 5. the map written: T2[a][k] / norm_factor for rows a = 0 and 2, -(T2[1][k] / norm_factor) for row 1.
 *   Step 5 is the constant matrix diag(1, -1, 1): it takes the camera point the annotation gives a pixel, (x, y, z) of scene[0..5], to the
 *   coordinate point (x', y', z) of scene[7..12] the renderer inverts.  The two differ by the image row's flip (v1 = row * 2 / H - 1 against
 *   v = (H - row) * 2 / H - 1), so x' = x and y' = -y for a projection without skew whose principal point is the image centre (projMat[:2,
 *   :2] diagonal, projMat[1][2] = 0: PyBullet's computeProjectionMatrixFOV, the reference's camera); R_l = -A_l of ancsh_pose_scene_build
 *   is the same statement for the eye point.
 *   A link gets an all-NaN map -- the renderer drops its triangles whole -- when it is not used (rank -1), its part is outside [0, K), one of
 *   its pose's 13 values is not finite, or the frame's norm factor is 0 or not finite.  Links >= nlinks read 0, as in the frame's table.
 *   One thread per (frame, variant, link), the grid a function of nframes alone; no host sync, no allocation: graph-capturable.  nframes == 0
 *   launches nothing and returns 0.  Checked before any launch: 0 <= nframes <= 32767 (the renderer takes 65535 frames), 1 <= K <= 8, rig_ld
 *   == ANCSH_RIG_WIDTH(K), ld >= 26, 0 <= pixel_capacity < 2^29, null pointers, the alignments (doubles 8 bytes, the others 4).
 *
 * ancsh_reproject_compare_rec: the pixel comparison, ONE launch behind the renderer and behind the record's poison step.
 *   obs_depth, obs_labels (pixel_capacity) : the pair the annotation read (with a sensor: the degraded pair);  pred_depth, pred_labels (2 *
 *   pixel_capacity) : what the renderer wrote for render_out / geom_out;  geom, scene : the frame's own;  carried (nframes, K, ld) float64 : the
 *   record row so far, columns 0..25 the two poses;  wide (nframes, K, ld + ANCSH_REPROJECTION_WIDTH) float64 : the output, a buffer of its own.
 *   A pixel is OBSERVED part j when its label names a used link (rank >= 0) whose part is j and its depth is usable by the annotation's rule
 *   (uint16: d != 0; float32: 0 < d < +inf); PREDICTED part j likewise on the predicted crop of the variant.  Over the pixels that are part j
 *   in both, d = ((double)pred - (double)obs) * depth_scale (scene[6]).  Row (f, j) of wide: columns 0..ld-1 = carried, bit for bit, then
 *     +0 n_obs   +1 n_pred   +2 n_both   +3 IoU = n_both / (n_obs + n_pred - n_both), NaN when the union is empty   +4 mean |d|   +5 RMS d
 *     +6 max |d|   +7 mean d (positive: the prediction lies behind the observation)      -- +1..+7 for the baseline pose --
 *     +8..+14 the same seven for the nonlinear pose.
 *   uint16 depths: S1 = sum |dq|, S = sum dq, S2 = sum dq^2 and the maximum over the integer quanta dq = pred - obs are int64, exact in any
 *   order, and converted once: mean |d| = ((double)S1 * depth_scale) / n_both, RMS = sqrt((double)S2 / n_both) * depth_scale, max = (double)max
 *   * depth_scale, mean = ((double)S * depth_scale) / n_both.  float32 depths: the float64 sums of |d|, d and d * d are added in a fixed order
 *   -- thread t of 256 adds pixels t, t + 256, ... of the crop in that order, a wave adds its lanes with xor shuffles of 32, 16, 8, 4, 2, 1,
 *   the four waves are added in wave order --, mean |d| = sum / n_both, RMS = sqrt(sum / n_both), mean likewise: the same bytes every run.
 *   NaN rules: a variant whose pose (13 values) is not finite has NaN in its seven columns; n_both == 0 gives NaN in the four depth columns;
 *   +0 is NaN when both poses are not finite -- so a frame whose record is poisoned, which includes every frame without rows, has NaN in all
 *   15.  A frame whose crop the depth entries refuse counts no pixel.
 *   One workgroup per (part, variant, frame); no atomics, no host sync, no allocation: graph-capturable.  nframes == 0 launches nothing and
 *   returns 0.  Checked before any launch: 0 <= nframes <= 32767, 1 <= K <= 8, depth_type, 0 <= pixel_capacity < 2^29, ld >= 26, null
 *   pointers, the alignments, carried != wide. */
#define ANCSH_REPROJECTION_WIDTH 15
int ancsh_reproject_scene_build(int nframes, int K, const double *render, const double *scene, const double *rig, int rig_ld,
                                const float *norm_factor, const double *record, int ld, const int *geom, long pixel_capacity,
                                double *render_out, int *geom_out, void *stream);
int ancsh_reproject_compare_rec(int nframes, int K, int depth_type, const void *obs_depth, const unsigned char *obs_labels,
                                long pixel_capacity, const void *pred_depth, const unsigned char *pred_labels, const int *geom,
                                const double *scene, const double *carried, int ld, double *wide, void *stream);

/* Render-and-compare ICP: the poses of a record refined on the depth frame, two entries around ancsh_reproject_scene_build and the unchanged
 * renderer (no new ABI number: callers detect them by their symbols).  Each (frame f, part j, pose v: 0 the baseline pose, 1 the nonlinear
 * pose) is refined on its own.  A pose is [R (9) row-major | s | t (3)], part NOCS -> the scaled cloud, c = s R x + t; R and t are refined, s
 * is carried.  The caller loops, pass = 0 .. iters:  ancsh_reproject_scene_build on the working poses, the renderer on the 2 * nframes
 * predicted frames, ancsh_refine_pass (is_last = 1 on pass == iters, which only evaluates);  then ancsh_refine_rec once.
 *
 * ancsh_refine_pass: one Gauss-Newton pass, ONE launch.
 *   verts, tris, tri_link, V, T : the mesh the renderer drew (a library: all of it; a z-buffer key names a global triangle);
 *   obs_depth, obs_labels (pixel_capacity) : the pair the annotation read;  pred_zbuf, pred_depth, pred_labels (2 * pixel_capacity) : what the
 *   renderer left for the working poses' tables, the z-buffer included: key = (bits of the float32 depth) << 32 | triangle;
 *   geom, scene (nframes, ..) : the frame's own;  pred_render (2 * nframes, ANCSH_RENDER_WIDTH) : ancsh_reproject_scene_build's tables for
 *   pose_in;  norm_factor (nframes) float32;  params : ONE table of ANCSH_REFINE_PARAMS = 8 float64 for the launch:
 *     [0] iters (the caller's; not read)  [1] max_dist  [2] min_cos  [3] damping  [4] max_angle, radians  [5] min_pixels  [6..7] reserved, 0;
 *   pose_in (nframes, K, ld_in) float64, ld_in >= 26 : columns 0..25 the two working poses (pass 0 reads the record itself);
 *   pose_out (nframes, K, 26) : the updated poses, a buffer of its own;  best (nframes, K, 2, 18) : the running best block, written on pass 0
 *   and read and written on later passes;  sums (nframes, K, 2, ANCSH_REFINE_SUMS = 32) : what this pass added up.
 * Everything is float64, evaluated in exactly the written order (no contraction); dot(a, b) = (a0 b0 + a1 b1) + a2 b2, |a| = sqrt(dot(a, a)).
 *   Space: the scaled cloud.  With nf = (double)norm_factor[f], a camera point (x', y', z) is the cloud point (nf x', nf (-y'), nf z).  Crop
 *   pixel (i, jj), row = row0 + i, col = col0 + jj, u = (C00 col + C01 row) + C02, w = (C10 col + C11 row) + C12 (scene[7..12]):  a depth z
 *   gives the camera point (z u, z w, z).  Observed point q: z = (double)d_obs * depth_scale (scene[6]);  predicted point p: z = (double) the
 *   float32 in the key's upper half.  Normal n: the key's triangle t, its link l = tri_link[t] and that link's map M of pred_render; a vertex
 *   (v0, v1, v2) -> m_a = ((M[a][0] v0 + M[a][1] v1) + M[a][2] v2) + M[a][3] -> the cloud as above;  e1 = B - A, e2 = C - A, n = e1 x e2
 *   (n0 = e1_1 e2_2 - e1_2 e2_1, cyclic), n = n / |n|, negated when dot(n, q) > 0.  |n| == 0 or not finite, t >= T, a vertex index outside
 *   [0, V) or a link outside [0, 16) skips the pixel.
 *   A pixel is OBSERVED for part j by ancsh_reproject_compare_rec's rule, and USED when the predicted pixel is part j by the same rule and
 *   |p - q| <= max_dist and |dot(n, q)| / |q| >= min_cos.  Centre c_a = s ((R[a][0] 0.5 + R[a][1] 0.5) + R[a][2] 0.5) + t_a.  Per used pixel r =
 *   dot(n, p - q), pc = p - c, J = [pc x n | n];  A = sum J J^T (upper triangle, row-major: 21 values), b = sum J r, sum r^2, n_used, n_obs.
 *   Order of addition: thread t of 256 adds pixels t, t + 256, ... of the crop in that order, a wave adds its lanes with xor shuffles of 32,
 *   16, 8, 4, 2, 1, the four waves are added in wave order: no atomics, the same bytes every run.
 *   sums row: [A (21) | b (6) | sum r^2 | n_used | n_obs | C | solved].  Cost C = (sum r^2 + (max_dist max_dist) (n_obs - n_used)) / n_obs, the
 *   truncated quadratic over the observed pixels; NaN when n_obs == 0.
 *   best row: [R (9) | s | t (3) | cost_start | cost_best | n_used at the best pose | best_pass | passes_solved].  Pass 0 writes pose_in and its
 *   C; a later pass replaces pose, cost_best, n_used and best_pass when its C is strictly lower (a NaN never is).
 *   The solve (skipped when is_last or n_used < min_pixels): A_kk = A_kk + (damping A_kk + 1e-12);  Cholesky A = L L^T row by row, s = A_ij,
 *   s = s - L_ik L_jk for k = 0 .. j - 1, L_ii = sqrt(s), L_ij = s / L_jj;  L y = -b forwards (s = (0 - b_i), s = s - L_ik y_k, y_i = s /
 *   L_ii), L^T xi = y backwards (k ascending from i + 1).  It FAILS when a pivot s is not > 0 or not finite, or a value of xi is not finite.
 *   xi = (w, dt): when |w| > max_angle or |dt| > max_dist all six are multiplied by the smaller of max_angle / |w| and max_dist / |dt| (of
 *   those that apply).  h = w / 2, qn = sqrt(((1 + h0 h0) + h1 h1) + h2 h2), the unit quaternion (1 / qn, h / qn) = (qw, x, y, z) and its
 *   matrix dR = [1 - 2 (y y + z z), 2 (x y - qw z), 2 (x z + qw y); 2 (x y + qw z), 1 - 2 (x x + z z), 2 (y z - qw x); 2 (x z - qw y),
 *   2 (y z + qw x), 1 - 2 (x x + y y)] -- sqrt and division only.  R'[a][k] = (dR[a][0] R[0][k] + dR[a][1] R[1][k]) + dR[a][2] R[2][k];
 *   t'_a = (dot(dR[a], t - c) + c_a) + dt_a;  s' = s.  solved = 1 and passes_solved grows by one; otherwise solved = 0 and pose_out = pose_in.
 *   NaN rules: a pose with a value that is not finite, or a norm factor that is 0 or not finite, has NaN in its 18 best values and its sums
 *   (solved = 0), and passes through pose_out as it came.
 *   One workgroup per (part, pose, frame); no host sync, no allocation: graph-capturable.  nframes == 0 launches nothing and returns 0.
 *   Checked before any launch: 0 <= nframes <= 32767, 1 <= K <= 8, depth_type, 0 <= pixel_capacity < 2^29, 0 <= T, V < 2^24, 0 <= pass <=
 *   ANCSH_REFINE_MAX_ITERS, is_last in {0, 1}, ld_in >= 26, null pointers, the alignments, pose_in != pose_out.
 *
 * ancsh_refine_rec: best (nframes, K, 2, 18) and the record row so far, carried (nframes, K, ld), -> wide (nframes, K, ld +
 *   ANCSH_REFINE_WIDTH): columns 0..ld-1 = carried bit for bit, then the baseline pose's best row and the nonlinear pose's.  ONE launch.
 *   Checked before any launch: 0 <= nframes <= 32767, 1 <= K <= 8, 26 <= ld <= 4096, null pointers, 8-byte alignments, carried != wide. */
#define ANCSH_REFINE_WIDTH 36
#define ANCSH_REFINE_SUMS 32
#define ANCSH_REFINE_PARAMS 8
#define ANCSH_REFINE_MAX_ITERS 8
int ancsh_refine_pass(int nframes, int K, int depth_type, const float *verts, const int *tris, const int *tri_link, int V, int T,
                      const void *obs_depth, const unsigned char *obs_labels, long pixel_capacity, const unsigned long long *pred_zbuf,
                      const void *pred_depth, const unsigned char *pred_labels, const int *geom, const double *scene,
                      const double *pred_render, const float *norm_factor, const double *params, int pass, int is_last,
                      const double *pose_in, int ld_in, double *pose_out, double *best, double *sums, void *stream);
int ancsh_refine_rec(int nframes, int K, const double *best, const double *carried, int ld, double *wide, void *stream);

/* The silhouette term of render-and-compare ICP, two entries beside the two above (no new ABI number: callers detect them by their symbols).
 * Point-to-plane on same-pixel pairs does not see a part that hangs over the edge of what the camera saw of it; these rows pull it back.
 * The loop becomes: ancsh_silhouette_field once (the observed pair does not change between passes), then pass = 0 .. iters:
 * ancsh_reproject_scene_build, the renderer, ancsh_refine_pass_sil; then ancsh_refine_rec, unchanged.
 *
 * ancsh_silhouette_field: ONE launch.  For every frame f, part j and crop pixel (i, jj): the nearest pixel (i', jj') of the same crop that is
 *   OBSERVED for part j (ancsh_reproject_compare_rec's rule), nearest by (di di + dj dj, i', jj') in that order, di = i' - i, dj = jj' - jj,
 *   all in integers: among equal distances the lower row, then the lower column.
 *   field (K, pixel_capacity) int32: part j's plane is field + j * pixel_capacity, and the word of crop pixel (i, jj) of frame f lies at the
 *   pixel's own address geom[f].start + i * w + jj:  word = (di & 0xffff) | (dj & 0xffff) << 16, two's-complement 16-bit halves.  The SENTINEL
 *   di = dj = -32768 (word 0x80008000) stands for a part without an observed pixel in the frame, and for every pixel of a crop taller or
 *   wider than 32767 pixels.  Words outside the crops are not written.  4 bytes per pixel and part.
 *   One workgroup per (part, one of 8 row-band workers, frame); no atomics, the same bytes every run; no host sync, no allocation:
 *   graph-capturable.  nframes == 0 launches nothing and returns 0.  Checked before any launch: 0 <= nframes <= 32767, 1 <= K <= 8,
 *   depth_type, 0 <= pixel_capacity < 2^29, null pointers, the alignments (obs_depth its element, geom and field 4, scene 8 bytes).
 *
 * ancsh_refine_pass_sil: ancsh_refine_pass with the term, ONE launch.  ancsh_refine_pass's arguments, and field (above) behind params;
 *   params : ONE table of ANCSH_REFINE_SIL_PARAMS = 16 float64: [0..7] as above, [8] weight > 0, [9] dist > 0 (the scaled cloud's unit),
 *   [10] slack >= 0 (pixels), [11..15] reserved, 0;  sums (nframes, K, 2, ANCSH_REFINE_SIL_SUMS = 36).
 *   Every rule of ancsh_refine_pass holds for the pixels it uses (the DEPTH rows): used pixels, normals, the centre, the order of addition,
 *   the solve, the clamp, the quaternion update, the NaN rules and best-of.  In addition a pixel is an OVERHANG pixel of (part j, pose v)
 *   when the predicted pixel is part j and the observed pixel is not part j and either is no part at all (background and holes read the
 *   same) or is another part with (double)d_obs * depth_scale > z_p, z_p = (double) the float32 in the key's upper half.  (Another part at
 *   or in front of the prediction is an occlusion: skipped.)  With the pixel's field word (di, dj):  skipped -- it costs nothing -- when the
 *   word is the SENTINEL or (double)(di di + dj dj) <= slack slack.  Otherwise row = row0 + i, col = col0 + jj, row' = row0 + i + di, col' =
 *   col0 + jj + dj (integers, then converted), u, w from (row, col) and u', w' from (row', col') as above;  p = cloud(z_p u, z_p w, z_p),
 *   p' = cloud(z_p u', z_p w', z_p);  dvec_a = p_a - p'_a (its z component is exactly 0);  m = |dvec|.  m > 0 fails (NaN included): skipped.
 *   m > dist: the pixel is FAR, n_far grows by one, no row.  Otherwise g = dvec / m, r = weight m, pc = p - c, J = [weight (pc x g)_0,
 *   weight (pc x g)_1, weight (pc x g)_2, weight g_0, weight g_1, weight g_2] ((pc x g)_0 = pc_1 g_2 - pc_2 g_1, cyclic): the row adds
 *   J_x J_y into A and J_x r into b exactly like a depth row, m m into sum m^2, and n_sil grows by one.  A pixel is a depth row or an
 *   overhang pixel, never both, so the order of addition is ancsh_refine_pass's: a thread's pixels in order, xor shuffles, waves in order.
 *   The row is linearised at fixed image geometry: it ignores that a change of the part's depth moves its silhouette in the image.
 *   sums row: [A (21) | b (6), both with the silhouette rows | sum r^2, n_used (the depth rows') | n_obs | C | solved | sum m^2 | n_sil |
 *   n_far | 0].  C = ((sum r^2 + (max_dist max_dist) (n_obs - n_used)) + (weight weight) (sum m^2 + (dist dist) n_far)) / n_obs; NaN when
 *   n_obs == 0.  n_obs does not depend on the pose, so a part's poses stay comparable, and a pose cannot lower its cost by overhanging.
 *   The solve runs when n_used + n_sil >= min_pixels.  best row: as above (n_used: the depth rows').  NaN rules: as above, sums[31] and
 *   sums[35] are 0.  Checked before any launch: ancsh_refine_pass's checks, field not null and 4-byte aligned. */
#define ANCSH_REFINE_SIL_SUMS 36
#define ANCSH_REFINE_SIL_PARAMS 16
int ancsh_silhouette_field(int nframes, int K, int depth_type, const void *obs_depth, const unsigned char *obs_labels, long pixel_capacity,
                           const int *geom, const double *scene, int *field, void *stream);
int ancsh_refine_pass_sil(int nframes, int K, int depth_type, const float *verts, const int *tris, const int *tri_link, int V, int T,
                          const void *obs_depth, const unsigned char *obs_labels, long pixel_capacity, const unsigned long long *pred_zbuf,
                          const void *pred_depth, const unsigned char *pred_labels, const int *geom, const double *scene,
                          const double *pred_render, const float *norm_factor, const double *params, const int *field, int pass, int is_last,
                          const double *pose_in, int ld_in, double *pose_out, double *best, double *sums, void *stream);

/* The joint step of render-and-compare ICP: an object's parts solved TOGETHER through their joints, one entry launched directly behind
 * ancsh_refine_pass[_sil] in every pass (no new ABI number: callers detect it by its symbol).  The pass refines each (frame, part, pose) on its
 * own, so a part that shows one flat face slides along it, a part below min_pixels is not moved, and nothing keeps a hinge's two sides
 * together.  This entry reads the 6 x 6 normal equations the pass left per part, adds rows that keep every revolute and prismatic joint's two
 * sides on one axis, solves the 6 K system, overwrites the poses the pass wrote, and keeps the best-of per OBJECT.  The loop becomes, pass = 0 ..
 * iters: ancsh_reproject_scene_build, the renderer, ancsh_refine_pass[_sil], ancsh_refine_joint_step; then ancsh_refine_rec, unchanged.
 *
 * ancsh_refine_joint_step: ONE launch, one workgroup of one wave per (pose v, frame f).
 *   kin (ninst, ANCSH_KIN_WIDTH) : the object's kinematic table(s); the frame's instance is value [9] of its pred_render row (0 for a single
 *   object), as the *_lib entries carry it;  scene, pred_render, norm_factor, pass, is_last, pose_in, ld_in : what the pass of this `pass` was
 *   given;  params : ONE table of ANCSH_REFINE_JOINT_PARAMS = 24 float64: [0..7] ancsh_refine_pass's, [8..15] ancsh_refine_pass_sil's (all 0
 *   without the term; not read here), [16] weight > 0, [17] axis_length >= 0 (the scaled cloud's unit), [18..23] reserved, 0;
 *   sums (nframes, K, 2, sums_ld), sums_ld = 32 or 36 (40: below) : what that pass wrote;  pose_out (nframes, K, 26) and best (nframes, K, 2, 18) : what
 *   that pass wrote, overwritten here;  state (nframes, K, 2, 18) : this entry's own shadow of the best block, written on pass 0, read and
 *   written later;  obj (nframes, 2, ANCSH_REFINE_OBJ = 8) : the object's row, likewise;  xi (nframes, 2, 48) or NULL : the clamped step, for
 *   debugging (0 where nothing was solved and behind 6 K).
 * Everything is float64 in exactly the written order (no contraction), with sqrt and division only; dot, |a|, the centre c_j, the cloud map
 * (x', y', z) -> nf (x', -y', z) and the part of a link are ancsh_refine_pass's.
 *   LIVE parts: part j is live when its 13 pose values are finite and nf is finite and not 0.  Its rows n_j = sums[28] (+ sums[33] when
 *   sums_ld = 36).  With n_j < min_pixels its A_j and b_j count as 0.  nbar = (sum of n_j) / (their number) over the live parts with n_j >=
 *   min_pixels, j ascending; with no such part nothing is solved.  w2n = (weight weight) nbar.
 *   Link maps: M_l = the 3 x 4 map of link l in the pose's pred_render row;  C_l(x) = cloud(m), m_a = ((M[a][0] x0 + M[a][1] x1) + M[a][2] x2) +
 *   M[a][3];  D_l(d) = u / |u| with u = (m_0, -m_1, m_2), m_a = (M[a][0] d0 + M[a][1] d1) + M[a][2] d2.
 *   ACTIVE joints: link l, 1 <= l < nlinks (scene[14]), of the instance's table with parent p (an integer in [0, l)) and kind 1 or 2, whose
 *   parts a = part(l) and b = part(p) are two different live parts of [0, K).  (A chain through a link of no part is not bridged; fixed joints
 *   add nothing.)  An instance outside [0, ninst), a parent outside [0, l) or a value that is no integer makes no joint.  With T = T_l and
 *   axis = the joint's axis (kin link values 4..15, 16..18):  x_c = C_l(0);  x_p = C_p(T[:, 3]);  u_c = D_l(axis);  u_p = D_p(T[:, :3] axis),
 *   (T[:, :3] d)_i = (T[i][0] d0 + T[i][1] d1) + T[i][2] d2.  At poses that reproduce the frame's own tables all four agree to rounding.
 *   Rows r0 + G xi, xi_j = (w_j, d_j) the step of part j about c_j; rows(e, h, r, sc, id): r0 = sc r;  G_a = [-[sc e]x | id I],
 *   G_b = [[sc h]x | -id I], [e]x = {0 -e2 e1; e2 0 -e0; -e1 e0 0}.
 *     position : rows(x_c - c_a, x_p - c_b, x_c - x_p, 1, 1);   direction : rows(u_c, u_p, u_c - u_p, axis_length, 0).
 *     Revolute: position, direction.  Prismatic: the position rows multiplied on the left by P = I - u_p u_p^T (P_ik = d_ik - u_p,i u_p,k;
 *     (P G)_ic = (P_i0 G_0c + P_i1 G_1c) + P_i2 G_2c, r0 likewise), the direction rows, and the direction rows of a second direction b = axis x
 *     e_k / |axis x e_k|, k the index of the smallest |axis_k| (ties: the lowest), taken through both links as the axis is: 9 rows.
 *     A joint with a row value r0 that is not finite, or a direction of length 0, is not active.
 *   The system, n = 6 K:  H = blockdiag(A_j, its diagonal damped as the pass damps it: A_kk + (damping A_kk + 1e-12)), g = (b_j); a part that
 *   is not live has the identity block and g = 0.  Then joint after joint, l ascending, with the 12 columns (a's six, b's six):  H_pq = H_pq +
 *   w2n t, t = 0 + G_0p G_0q + G_1p G_1q + ... (rows ascending);  g_p = g_p + w2n t, t = 0 + G_0p r0_0 + ...
 *   Cholesky H = L L^T:  element (i, j), i >= j, is s = H_ij, s = s - L_ik L_jk for k = 0 .. j - 1 (ascending, in one thread: the bytes do not
 *   depend on how the elements are spread over the lanes), L_jj = sqrt(s), L_ij = s / L_jj.  L y = -g: s = 0 - g_i, s = s - L_ik y_k for k
 *   ascending, y_i = s / L_ii.  L^T xi = y: s = y_i, s = s - L_ki xi_k for k = n - 1 DOWN TO i + 1, xi_i = s / L_ii.  It FAILS when a pivot s is
 *   not > 0 or not finite, or a value of xi is not finite.
 *   Clamp: ONE factor for the object: f = 1, then for the live parts, j ascending: |w_j| > max_angle and max_angle / |w_j| < f: f = that;
 *   |d_j| > max_dist and max_dist / |d_j| < f: f = that.  xi = xi f when f < 1.  Update: ancsh_refine_pass's quaternion update of every live
 *   part with (w_j, d_j), written to pose_out.
 *   Nothing to solve -- no active joint, no nbar, is_last, or a failed solve --: pose_out stays what the pass wrote.
 *   Object cost: num = sum C_j n_obs_j, den = sum n_obs_j over the live parts with n_obs_j > 0 (C_j = sums[30], n_obs_j = sums[29], j
 *   ascending); with an active joint and nbar: num = num + w2n (sum over the joints, l ascending, of (0 + r0_0 r0_0 + r0_1 r0_1 + ...));
 *   Cobj = num / den, NaN when den = 0.
 *   Best-of, per OBJECT: on pass 0, or when Cobj is strictly lower than the object's cost_best (a NaN never is), the shadow `state` takes the
 *   13 values of ALL K parts' pose_in, their own C_j (column 14; on pass 0 column 13 too) and n_used_j (15) -- NaN in 13..15 for a part that
 *   is not live -- and the pass number.  Every pass then writes columns 16 = the object's best_pass and 17 = the object's passes_solved (the
 *   passes in which a solve moved a pose of the object: this entry's, or -- where it solved nothing -- a part's own) and rewrites `best` from
 *   the shadow; what the pass wrote there is ignored.  A part that is not live in this pass reads 18 NaN.  So cost_best <= cost_start holds for
 *   the OBJECT (obj), no longer for each part.
 *   obj row: [cost_start | cost_best | best_pass | passes_solved | this pass's Cobj | active joints | 1 when this entry solved | sqrt((sum of
 *   the joints' squared position residuals |r0_0..2|^2) / joints), NaN without one].
 *   No atomics, the same bytes every run; no host sync, no allocation: graph-capturable.  nframes == 0 launches nothing and returns 0.
 *   Checked before any launch: 0 <= nframes <= 32767, 1 <= K <= 8, 1 <= ninst <= 65535, 0 <= pass <= ANCSH_REFINE_MAX_ITERS, is_last in {0,
 *   1}, ld_in >= 26, sums_ld in {32, 36, 40}, null pointers (xi may be NULL), the alignments (norm_factor 4, everything else 8 bytes), pose_in !=
 *   pose_out, best != state. */
#define ANCSH_REFINE_JOINT_PARAMS 24
#define ANCSH_REFINE_OBJ 8
int ancsh_refine_joint_step(int nframes, int K, const double *kin, int ninst, const double *scene, const double *pred_render,
                            const float *norm_factor, const double *params, int pass, int is_last, const double *pose_in, int ld_in,
                            const double *sums, int sums_ld, double *pose_out, double *best, double *state, double *obj, double *xi,
                            void *stream);

/* The coverage term of render-and-compare ICP, two entries beside those above (no new ABI number: callers detect them by their symbols).  The
 * silhouette term is one-sided: a predicted pixel that hangs over the observed part's edge is pulled back, but an observed pixel of the part
 * that the prediction leaves BARE is only charged max_dist^2, a flat charge that pulls nothing.  These rows pull the part over such pixels.
 * They need the silhouette term.  The loop becomes: ancsh_silhouette_field once, then pass = 0 .. iters: ancsh_reproject_scene_build, the
 * renderer, ancsh_coverage_field, ancsh_refine_pass_cov[, ancsh_refine_joint_step]; then ancsh_refine_rec, unchanged.
 *
 * ancsh_coverage_field: ONE launch, directly behind the renderer in every pass: ancsh_silhouette_field's computation on the PREDICTED pair.
 *   pred_depth, pred_labels : the renderer's buffers of 2 * pixel_capacity pixels, pose v's half first pixel v * pixel_capacity;  geom_out (2 *
 *   nframes, 5) : ancsh_reproject_scene_build's description of the 2 * nframes predicted frames, row v * nframes + f = pose v of frame f;
 *   scene (nframes, 240) : frame row v * nframes + f reads scene row f.  For every predicted frame, part j and crop pixel (i, jj): the nearest
 *   pixel of the same crop that is PREDICTED for part j (ancsh_reproject_compare_rec's rule on the predicted pair), by ancsh_silhouette_field's
 *   order (di di + dj dj, then the lower row, then the lower column, in integers), in its word format and with its SENTINEL.
 *   cover (K, 2 * pixel_capacity) int32: part j's plane is cover + j * 2 * pixel_capacity, and a crop pixel's word lies at the pixel's own
 *   address in the predicted buffers, geom_out[v * nframes + f].start + i * w + jj.  Words outside the crops are not written.  8 bytes per
 *   pixel of pixel_capacity and part.  The same kernel, the same grid per frame, the same bytes every run; graph-capturable.  nframes == 0
 *   launches nothing and returns 0.  Checked before any launch: ancsh_silhouette_field's checks (pixel_capacity is the observed buffers', 0 <=
 *   pixel_capacity < 2^29; a crop must lie inside [0, 2 * pixel_capacity) or it counts as no crop).
 *
 * ancsh_refine_pass_cov: ancsh_refine_pass_sil with the term, ONE launch.  ancsh_refine_pass_sil's arguments, and cover (above) behind field;
 *   params : ONE table of ANCSH_REFINE_COV_PARAMS = 32 float64: [0..7] ancsh_refine_pass's, [8..15] ancsh_refine_pass_sil's, [16..23] the
 *   joint step's (all 0: the joint step is off; not read here), [24] weight_c > 0, [25] dist_c > 0 (the scaled cloud's unit), [26] slack_c >= 0
 *   (pixels), [27..31] reserved, 0;  sums (nframes, K, 2, ANCSH_REFINE_COV_SUMS = 40).
 *   Every rule of ancsh_refine_pass_sil holds for the depth rows and the overhang pixels.  In addition crop pixel a = (i, jj) is a GAP pixel of
 *   (part j, pose v) when the observed pixel is part j and the predicted pixel is not part j.  A pixel is a depth row, an overhang pixel or a
 *   gap pixel, never two of them, so the order of addition is unchanged.  For a gap pixel, z_o = (double)d_obs * depth_scale, in this order (a
 *   skipped pixel costs nothing more than the max_dist^2 it is charged as a missed pixel):
 *   1. the predicted pixel is another part: z_q = (double) the float32 in its key's upper half;  !(z_q > z_o): the prediction puts another
 *      part in front -- skipped (the overhang's occlusion rule, mirrored).
 *   2. the cover word (di, dj) of part j at this pixel in pose v's half, cover[j * 2 * pixel_capacity + v * pixel_capacity + start + i * w +
 *      jj]:  the SENTINEL (the part drew no pixel in this frame): skipped;  (double)(di di + dj dj) <= slack_c slack_c: skipped.  (A word that
 *      points outside the crop -- never one of ancsh_coverage_field's -- is skipped.)
 *   3. a2 = (i + di, jj + dj), the nearest predicted pixel of the part;  z_2 = (double) the float32 in a2's key's upper half;  u, w from (row,
 *      col) = (row0 + i, col0 + jj) and u2, w2 from (row + di, col + dj), integers converted afterwards, as the overhang row does.
 *   4. pn = cloud(z_2 u2, z_2 w2, z_2), the predicted surface point;  pt = cloud(z_2 u, z_2 w, z_2), the same depth on the bare pixel's ray;
 *      dvec_a = pn_a - pt_a (its z component is exactly 0);  m = |dvec|.  m > 0 fails (NaN included): skipped.
 *   5. m > dist_c: the pixel is FAR, n_cfar grows by one, no row.
 *   6. otherwise g = dvec / m, r = weight_c m, pc = pn - c, J = weight_c [pc x g | g] in the overhang row's component order: J_x J_y into A, J_x
 *      r into b, m m into sum m_c^2, and n_cov grows by one.
 *   The row, like the overhang's, is linearised at fixed image geometry; it moves R and t only (s and q are carried).
 *   sums row: [0..35] ancsh_refine_pass_sil's, A and b with the coverage rows | [36] sum m_c^2 | [37] n_cov | [38] n_cfar | [39] 0.
 *   C = (ancsh_refine_pass_sil's numerator + (weight_c weight_c) (sum m_c^2 + (dist_c dist_c) n_cfar)) / n_obs, added last; NaN when n_obs ==
 *   0.  The solve runs when (n_used + n_sil) + n_cov >= min_pixels.  NaN rules: as above; sums[31], sums[35] and sums[39] are 0.  The solve,
 *   the clamp, the quaternion update and best-of are ancsh_refine_pass's.  Checked before any launch: ancsh_refine_pass_sil's checks, cover
 *   not null and 4-byte aligned.
 *
 * ancsh_refine_joint_step accepts sums_ld == 40 and a 32-value table with joint values: n_j = (sums[28] + sums[33]) + sums[37]; it reads
 *   params [16] and [17] as of a 24-value table; everything else is as stated above. */
#define ANCSH_REFINE_COV_SUMS 40
#define ANCSH_REFINE_COV_PARAMS 32
int ancsh_coverage_field(int nframes, int K, int depth_type, const void *pred_depth, const unsigned char *pred_labels, long pixel_capacity,
                         const int *geom_out, const double *scene, int *cover, void *stream);
int ancsh_refine_pass_cov(int nframes, int K, int depth_type, const float *verts, const int *tris, const int *tri_link, int V, int T,
                          const void *obs_depth, const unsigned char *obs_labels, long pixel_capacity, const unsigned long long *pred_zbuf,
                          const void *pred_depth, const unsigned char *pred_labels, const int *geom, const double *scene,
                          const double *pred_render, const float *norm_factor, const double *params, const int *field, const int *cover,
                          int pass, int is_last, const double *pose_in, int ld_in, double *pose_out, double *best, double *sums, void *stream);

/* The scale unknown of render-and-compare ICP, one entry beside those above (no new ABI number: callers detect it by its symbol).  The loop
 * moves R and t of every (frame, part, pose) and carries s, the network's NOCS scale; a part that is too small is then pulled over its
 * observation by moving, not by growing.  The overhang rows (the part is drawn where the camera did not see it) and the gap rows (the camera
 * saw the part where nothing is drawn) observe size -- depth rows alone cannot tell scale from depth along the ray -- so with both pixel terms
 * on, this entry solves a seventh unknown sigma, the relative change of the part's size about its centre c.  The loop is the coverage loop
 * with ancsh_refine_pass_scale in ancsh_refine_pass_cov's place; the joint step is not combined with it.
 *
 * ancsh_refine_pass_scale: ancsh_refine_pass_cov with the unknown, ONE launch.  ancsh_refine_pass_cov's arguments, and behind cover:
 *   fitted (nframes, K, ld_fitted) float64, ld_fitted >= 26 : the record the loop started from; s_0 of pose v of part j of frame f is
 *   fitted[(f K + j) ld_fitted + 13 v + 9];
 *   params : ONE table of ANCSH_REFINE_SCALE_PARAMS = 48 float64: [0..31] ancsh_refine_pass_cov's ([16..23] all 0), [32] max_step in (0, 0.5],
 *   [33] max_total in [max_step, 1], [34..47] reserved, 0;  sums (nframes, K, 2, ANCSH_REFINE_SCALE_SUMS = 48).
 *   Every rule of ancsh_refine_pass_cov holds: which pixels give which rows, r and J = (J_0 .. J_5) of each, the centre, the cost C and
 *   best-of (so costs stay comparable with and without the unknown), n_rows = (n_used + n_sil) + n_cov >= min_pixels, is_last.  In addition
 *   every row has a seventh derivative Js, the row's r by sigma when a point x of the part moves as c + (1 + sigma) (x - c):
 *     depth row    : Js = dot(n, pc), pc = p - c;
 *     overhang row : Js = weight dot(g, pc), pc = p - c (that row's p and g);
 *     gap row      : Js = weight_c dot(g, pc), pc = pn - c (that row's pn and g);
 *   and adds, behind its J_x J_y and J_x r and in this order, J_x Js into A_xs (x = 0 .. 5), Js Js into A_ss and Js r into b_s.  These eight
 *   are accumulators 36..43 behind the coverage pass's 36: the same pixel order, xor-shuffle tree and wave order, no atomics.
 *   sums row: [0..39] ancsh_refine_pass_cov's | [40..45] A_0s .. A_5s | [46] A_ss | [47] b_s.
 *   The solve: the 7 x 7 system [A (6 x 6), A_xs; A_xs^T, A_ss] xi = -[b; b_s] in ancsh_refine_pass's written order with 7 in 6's place: every
 *   diagonal A_kk = A_kk + (damping A_kk + 1e-12), k = 0 .. 6; Cholesky row by row; L y = -b forwards; L^T xi = y backwards from row 6.  It
 *   FAILS when a pivot is not > 0 or not finite, or one of the seven values is not finite.  xi = (w, dt, sigma).
 *   Clamp: when |w| > max_angle or |dt| > max_dist or |sigma| > max_step, all SEVEN values are multiplied by f: f = 1; |w| > max_angle: f =
 *   max_angle / |w|; |dt| > max_dist and max_dist / |dt| < f: f = that; |sigma| > max_step and max_step / |sigma| < f: f = that.  Then sigma
 *   alone: lo = s_0 / (1 + max_total), hi = s_0 (1 + max_total), with s the working pose's:  s (1 + sigma) > hi: sigma = hi / s - 1;  else s (1
 *   + sigma) < lo: sigma = lo / s - 1.  A working s that is not > 0, or a kept s (1 + sigma) that is not finite or not > 0, FAILS the solve
 *   as well.
 *   Update: dR from w as in ancsh_refine_pass;  R' = dR R;  s' = s * (1.0 + sigma);  t'_a = ((1.0 + sigma) * dot(dR[a], t - c) + c_a) + dt_a:
 *   x' = c + (1 + sigma) dR (x - c) + d for every point x of the part.  With sigma = 0 and the scale sums 0 these are ancsh_refine_pass_cov's
 *   bytes.
 *   NaN rules: ancsh_refine_pass_cov's, sums[40..47] are NaN on that branch; a pose whose s_0 is not finite or not > 0 takes that branch too.
 *   Checked before any launch, in ancsh_refine_pass_cov's order and under the name refine_pass_scale: its checks, ld_fitted >= 26 behind ld_in,
 *   fitted not null and 8-byte aligned.  nframes == 0 launches nothing and returns 0. */
#define ANCSH_REFINE_SCALE_SUMS 48
#define ANCSH_REFINE_SCALE_PARAMS 48
int ancsh_refine_pass_scale(int nframes, int K, int depth_type, const float *verts, const int *tris, const int *tri_link, int V, int T,
                            const void *obs_depth, const unsigned char *obs_labels, long pixel_capacity, const unsigned long long *pred_zbuf,
                            const void *pred_depth, const unsigned char *pred_labels, const int *geom, const double *scene,
                            const double *pred_render, const float *norm_factor, const double *params, const int *field, const int *cover,
                            const double *fitted, int ld_fitted, int pass, int is_last, const double *pose_in, int ld_in, double *pose_out,
                            double *best, double *sums, void *stream);

/* The joint values q of a posed frame read off its part poses: ancsh_pose_scene_build's forward kinematics inverted on the predicted link
 * maps, ONE launch at the step's end (no new ABI number: callers detect it by its symbol).  The posed stream takes q in (pose[f][l]); this
 * entry reports it on the way out, per part and pose, with its error against the submitted value and how far the two sides of the joint are
 * from lying on one axis.  The reference has nothing here: its joint states (ancsh_joint_state_rec) measure part j against part 0 about the
 * network's own axis and know nothing of the object's kinematic tree.
 *   kin (ninst, ANCSH_KIN_WIDTH), pose (nframes, ANCSH_POSE_WIDTH) or NULL, render, scene, rig (rig_ld = ANCSH_RIG_WIDTH(K)), norm_factor,
 *     record (nframes, K, ld >= 26) : as ancsh_pose_scene_build[_lib], ancsh_reproject_scene_build and ancsh_refine_joint_step take them; the
 *     frame's instance is render[f][9] (0 for a single object), an integer in [0, ninst);
 *   refined (nframes, K, 2, 18) float64 or NULL : the refinement's kept poses (its best block: values 0..12 of a row are a pose);
 *   art (nframes, K, art_ld) float64, art_ld = 12 (ancsh_articulation_rec's block) or 20 (ancsh_joint_state_rec's);
 *   wide (nframes, K, art_ld + ANCSH_JOINT_VALUES_WIDTH = 24) float64, a buffer of its own : columns 0..art_ld-1 of row (f, j) = art's row, bit
 *     for bit (moved as 64-bit words: a NaN keeps its payload), the 24 columns below behind them.
 * WHICH JOINT row j reports: the bridging joint of part j, the lowest link l in [1, nlinks) such that its part (ancsh_reproject_scene_build's
 *   rule: the link is used and scene link value [1] lies in [0, K)) is j, its kind (kin link value [3]) is 1 or 2, its parent p (kin link
 *   value [2]) is an integer in [0, l), and the parent's part b is in [0, K) and is not j.  A row without such a joint -- the base part, a part
 *   behind a link of no part, a part whose joints are all fixed -- is NaN in all 24 columns; so is every row of a frame whose norm factor is 0
 *   or not finite or whose instance value is not an integer in [0, ninst).
 * LINK MAPS: B_l = [M_l | tau_l] is exactly what ancsh_reproject_scene_build writes for link l under its part's pose (its steps 1..5, the
 *   same device function).  Four pose groups g: record columns 0..12, record columns 13..25, refined[f][.][0][0..12], refined[f][.][1][0..12];
 *   the child link takes part j's pose and the parent link part b's pose, both from group g.
 * ARITHMETIC, float64 in exactly the written order (no contraction); dot(x, y) = (x0 y0 + x1 y1) + x2 y2, |x| = sqrt(dot(x, x)); Rt[a][k] =
 *   kin link value [4 + 4a + k], org_a = value [4 + 4a + 3], a = values [16..18] of link l:
 *     sigma_l = sqrt(S / 3), S = the nine squares M_l[a][k]^2 added to 0 in row-major order; sigma_p likewise;
 *     E[i][k] = ((M_p[0][i] M_l[0][k] + M_p[1][i] M_l[1][k]) + M_p[2][i] M_l[2][k]) / (sigma_p * sigma_l);
 *     G[i][k] = (Rt[0][i] E[0][k] + Rt[1][i] E[1][k]) + Rt[2][i] E[2][k];
 *     v = ((G21 - G12) / 2, (G02 - G20) / 2, (G10 - G01) / 2);   c = (((G00 + G11) + G22) - 1) / 2;
 *     d_i = tau_l[i] - (dot(M_p[i], org) + tau_p[i]);   ra_i = dot(Rt[i], a);   w_i = dot(M_p[i], ra);   u = w / |w|;
 *     revolute (kind 1):  q = atan2(dot(a, v), c);  Ga_i = dot(G[i], a), x = a x Ga = (a1 Ga2 - a2 Ga1, a2 Ga0 - a0 Ga2, a0 Ga1 - a1 Ga0),
 *       off_axis = atan2(|x|, dot(a, Ga));  gap = |d|;
 *     prismatic (kind 2): q = dot(d, u);  off_axis = atan2(|v|, c);  r_i = d_i - q u_i, gap = |r|;
 *     scale_ratio = sigma_l / sigma_p;   q_err = q - q_true, q_true = pose[f][l]; for a revolute joint q_err - 2 pi when it exceeds pi, else
 *     q_err + 2 pi when it lies below -pi (one conditional step: into [-pi, pi] for |q_true| <= pi).
 *   In exact arithmetic and for a record that reproduces the frame's own tables M_p^T M_l / (sigma_p sigma_l) = Rt Rj(q) and d = q u
 *   (prismatic) or 0 (revolute), J_l(q) = [Rj | tj] of ancsh_pose_scene_build: q is the submitted value, off_axis and gap vanish and the ratio
 *   is 1.  Lengths (a prismatic q, gap) are in the renderer's unit (camera = model), not the scaled cloud's: gap * norm_factor is the distance
 *   of the two sides in the cloud's unit, ancsh_refine_joint_step's hinge gap.  Angles are radians.
 * COLUMNS behind the carried row:  +0 link l   +1 kind   +2 parent_part b   +3 q_true   then per group g at +4 + 5 g:  q, q_err, off_axis,
 *   gap, scale_ratio.
 * NaN RULES: a group's five columns are NaN when the child's or the parent's pose (13 values) is not finite, or sigma_l, sigma_p or |w| is 0
 *   or not finite; refined == NULL: both refined groups are NaN; pose == NULL: q_true and every q_err are NaN.
 * One thread per (frame, part, group), the grid a function of nframes and K alone; every index read from a table is range-checked before it
 * addresses anything; no atomics, no host sync, no allocation: graph-capturable, the same bytes every run.  A few hundred double operations
 * per thread: the launch sits on the floor of a dependent graph node.  nframes == 0 launches nothing and returns 0.  Checked before any
 * launch: 0 <= nframes <= 32767, 1 <= K <= 8, ninst >= 1, rig_ld == ANCSH_RIG_WIDTH(K), ld >= 26, art_ld 12 or 20, null pointers (pose and
 * refined may be NULL), the alignments (doubles 8 bytes, norm_factor 4), art != wide. */
#define ANCSH_JOINT_VALUES_WIDTH 24
int ancsh_joint_values_rec(int nframes, int K, const double *kin, int ninst, const double *pose, const double *render, const double *scene,
                           const double *rig, int rig_ld, const float *norm_factor, const double *record, int ld, const double *refined,
                           const double *art, int art_ld, double *wide, void *stream);

/* Per-raw-point segmentation of a streamed batch: the FP module's upsampling rule (pointnet_util.py:219-229: 3-NN, inverse-distance
 * weights, three_interpolate) from each cloud's num_points sampled points to every one of its raw rows.  Cloud b owns raw rows
 * [offsets[b], offsets[b+1]) of `rows` (capacity x nchan float32, x y z first), norm factor norm_factor[b], sampled points P (nclouds,
 * num_points, 3) and the heads W (nclouds, num_points, K), nocs (.., 3K) of the NPCS network and gocs (.., gocs_channels = 3 or 3K) of
 * the ANCSH network.  For raw row r = (x, y, z):
 *   q = (x * nf, y * nf, z * nf), the f32 products ancsh_input_sample_stream writes into P (a sampled row is at distance 0 from its copy);
 *   its 3-NN among P[b] with ancsh_three_nn's arithmetic ((dx*dx + dy*dy) + dz*dz, no contraction) and (distance, index) order, and
 *   ancsh_three_nn_weights' weights; each needed channel interpolated in ancsh_three_interpolate's order;
 *   labels[r] (int32) = the first k of the largest interpolated W_k (np.argmax), -1 if q or any interpolated W channel is non-finite;
 *   values[r] (7 float32) = [W_label | nocs[3l..3l+2] | gocs[3l..3l+2], or gocs[0..2] when gocs_channels = 3]; all NaN when the label is -1.
 * Bit-equal to ancsh_three_nn_weights + ancsh_three_interpolate per cloud on (q, P[b]) followed by the selection.  Rows outside
 * [offsets[0], offsets[nclouds]) are left untouched, as is a cloud whose rows are empty or outside [0, capacity).  Graph-capturable: the
 * grid depends on (capacity, nclouds) only, every cloud size is read from device offsets; no host sync, no allocation.  Checked before
 * any launch: nclouds <= 65535, 1 <= K <= 8, gocs_channels in {3, 3K}, nchan >= 3, 0 <= capacity < 2^30, null pointers. */
int ancsh_raw_point_labels(int nclouds, int num_points, int K, int gocs_channels, int nchan, const float *rows, long capacity,
                           const int *offsets, const float *norm_factor, const float *P, const float *W, const float *nocs,
                           const float *gocs, int *labels, float *values, void *stream);

/* ---- test-time losses of predict_and_save (lib/network.py:430-498, lib/loss.py:54-182) ------- */

/* One launch per batch; ptrs = 16 device pointers {W (b,n,K), nocs (b,n,3K), gocs (b,n,3K)|NULL, heatmap (b,n), unitvec (b,n,3),
 * joint_axis (b,n,3), index (b,n,3), cls_gt (b,n) int32 (-1 allowed), joint_cls_gt (b,n) int32, nocs_gt (b,n,3),
 * gocs_gt (b,n,3)|NULL, mask_array (b,n,K), heatmap_gt (b,n), unitvec_gt (b,n,3), orient_gt (b,n,3), joint_cls_mask (b,n)}.
 * out (b, 5+K+3) = [nocs_loss, gocs_loss, heatmap_loss, unitvec_loss, orient_loss | miou_loss[K] | index_loss[3]] per cloud,
 * i.e. loss_dict of compute_loss before collect_losses' batch means.  type_l: 0 = 'L2', 1 = 'L1' (cfg coord_regress_loss). */
int ancsh_test_losses(int b, int n, int K, int type_l, const void *const *ptrs, float *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ANCSH_HIP_H */
