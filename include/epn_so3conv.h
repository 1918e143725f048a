/*
 * include/epn_so3conv.h -- C ABI of libepn_so3conv.so (MI355X / gfx950).
 *
 * Drop-in boundary for the EPN SE(3) separable point-convolution hot path.  Every entry point is
 * `extern "C"`, takes plain DEVICE pointers + sizes + a HIP stream (passed as void*), launches
 * asynchronously on that stream, owns no memory and keeps no global state other than epn_set_kernel_policy (thread-safe) and the thread-local diagnostic
 * string behind epn_last_kernel.  Return
 * value: 0 on success, otherwise a hipError_t code (launch errors) or a negative EPN_E* code
 * (argument errors).  `epn_strerror` turns either into text.
 *
 * Each function names the reference interface it replaces (paths relative to the reference repo
 * nintendops/EPN_PointCloud).  The reference's pybind functions allocate their outputs; here the
 * CALLER allocates (the Python mirror in epn_pointcloud_amd/vgtk/cuda does it with torch).
 *
 * Layout notes
 *   xyz tensors are channel-major  [b,3,n]  exactly as the reference passes them.
 *   Feature tensors at THIS boundary are channels-last: feats_cl[b][p][a][c]  (the memory image of a
 *   torch tensor of logical shape [b,c,p,a] in torch.channels_last format).  The public nn.Module
 *   API keeps the reference's logical [b,c,p,a] shape.
 */
#ifndef EPN_SO3CONV_H
#define EPN_SO3CONV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EPN_EINVAL (-1)      /* bad size / unsupported shape                      */
#define EPN_EWORKSPACE (-2)  /* workspace pointer NULL or too small               */
#define EPN_ENULL (-3)       /* required pointer is NULL                          */

typedef void *epn_stream_t; /* hipStream_t; NULL = the null stream */

/* Integer revision of this binary interface: bumped whenever an EXISTING signature or struct layout changes (new entry
 * points alone do not bump it).  A host compares epn_abi_version() of the library it loaded with the EPN_ABI_VERSION of
 * the header it was compiled against and refuses to run on a mismatch -- revision 2 changed `epn_ball_query_f64`'s radius
 * from double to float and grew `struct epn_gemm_nt_problem`, which a caller built against revision 1 would not notice;
 * revision 3 (round 6) grew that struct again (`c_amax`)
 * (INTEGRATION.md "ABI revisions").  epn_pointcloud_amd/_lib.py performs exactly this check at load time. */
#define EPN_ABI_VERSION 3
int epn_abi_version(void);
const char *epn_version(void);
const char *epn_strerror(int code);
/* Diagnostic: the device kernel (exact template instance, "(anonymous namespace)::" removed, e.g.
 * "epn::gemm_nt_x3_kernel<4, 2, 2, 4, 2>") that the calling thread's most recent library call launched as its main
 * kernel -- what rocprofv3 will call it -- so a benchmark can attribute time without re-deriving the launchers' tile
 * choices.  Thread-local, cleared by the read; "" when nothing was launched since the last read.  The returned
 * pointer is valid until the thread's next call of this function. */
const char *epn_last_kernel(void);

/* Cross-check switch, the library's only process-wide state (a relaxed atomic; default 0): 0 = every entry point picks
 * its best kernel, 1 = the any-shape generic kernels everywhere (an independent on-device implementation used by the
 * parity tests).  Not for production use; set it before launching from other threads.  Any other value: EPN_EINVAL.
 * (Libraries built with -DEPN_TUNING -- `python -m epn_pointcloud_amd.build --tuning`, used by tools/ only -- also accept
 * 0x100|v .. 0x400|v, the A/B switches of the tuning tools: GEMM tile overrides, 0x401 = per-slot atomic scatter.) */
int epn_set_kernel_policy(int policy);

/* ------------------------------------------------------------------ index kernels ---------- */

/* Replaces vgtk.cuda.grouping.ball_query  (vgtk/vgtk/cuda/grouping_cuda.cpp:71-86, kernel
 * grouping_cuda_kernel.cu:67-113).  new_xyz f32[b,3,m], xyz f32[b,3,n] -> idx i32[b,m,nsample].
 * The kernel writes every slot (the reference zero-fills first, grouping_cuda.cpp:80-82). */
int epn_ball_query_f32(const float *new_xyz, const float *xyz, int b, int n, int m, float radius,
                       int nsample, int32_t *idx, epn_stream_t stream);

/* Replaces vgtk.cuda.grouping.furthest_point_sampling (grouping_cuda.cpp:160-174, kernel
 * grouping_cuda_kernel.cu:351-466).  xyz f32[b,3,n] -> idx i32[b,m].  The 1e10 `temp` buffer of
 * the reference lives in registers.  Requires 1 <= m, 1 <= n <= 32768 (EPN_EINVAL beyond: use
 * epn_fps_temp_f32, which keeps the running minima in a caller-provided `temp` f32[b,n] like the
 * reference kernel -- its strided loop has no size limit, grouping_cuda_kernel.cu:380-396 -- and
 * gives the same indices for every n). */
int epn_fps_f32(const float *xyz, int b, int n, int m, int32_t *idx, epn_stream_t stream);
int epn_fps_temp_f32(const float *xyz, int b, int n, int m, float *temp, int32_t *idx, epn_stream_t stream);

/* Replace vgtk.cuda.gathering.gather_points_forward / _backward (gathering_cuda.cpp:29-60,
 * kernels gathering_cuda_kernel.cu:43-98).  points f32[b,c,n], idx i32[b,m] -> out f32[b,c,m];
 * grad_out f32[b,c,m] -> grad_points f32[b,c,n] (zero-filled here, then scatter-added). */
int epn_gather_fwd_f32(const float *points, const int32_t *idx, int b, int c, int n, int m,
                       float *out, epn_stream_t stream);
int epn_gather_bwd_f32(const float *grad_out, const int32_t *idx, int b, int c, int n, int m,
                       float *grad_points, epn_stream_t stream);

/* fp64 dispatch of the same four extensions: the reference instantiates them for float AND double
 * (AT_DISPATCH_FLOATING_TYPES: grouping_cuda_kernel.cu:477 ball query, :638-726 FPS; gathering_cuda_kernel.cu:117,151).
 * Same semantics with double coordinates / features; indices stay int32.  epn_fps_f64 takes the reference's `temp`
 * buffer (f64[b,n], grouping_cuda.cpp:167-168; initialised to 1e10 here) because it keeps the running minima there, as the
 * reference kernel does -- fp64 sampling is a compatibility path, not a tuned one.  `radius` stays a FLOAT and is squared in
 * float before it is widened, as the reference's templated kernel does (`float radius`, `scalar_t radius2 = radius *
 * radius;`, grouping_cuda_kernel.cu:67,80; host side grouping_cuda.cpp:74). */
int epn_ball_query_f64(const double *new_xyz, const double *xyz, int b, int n, int m, float radius, int nsample,
                       int32_t *idx, epn_stream_t stream);
int epn_fps_f64(const double *xyz, int b, int n, int m, double *temp, int32_t *idx, epn_stream_t stream);
int epn_gather_fwd_f64(const double *points, const int32_t *idx, int b, int c, int n, int m, double *out,
                       epn_stream_t stream);
int epn_gather_bwd_f64(const double *grad_out, const int32_t *idx, int b, int c, int n, int m, double *grad_points,
                       epn_stream_t stream);

/* Patch extraction around keypoints: every point of ONE fragment within `radius` of a keypoint, resampled to n_sample
 * points.  Replaces the host path of the reference's 3DMatch loader -- scipy KDTree + query_ball_point per keypoint
 * (SPConvNets/datasets/match_3dmatch.py:154-177), then np.random.choice to input_num points
 * (vgtk/vgtk/pc/sample.py:16-36) -- whose selection is random and unordered; this is the library's own deterministic form
 * of the same semantics.
 *   pc f32[n,3] (row-major), kpts f32[k,3] -> idx i32[k,n_sample], counts i32[k], patches f32[k,n_sample,3].
 * For keypoint row q, with global row Q = kpt_row0 + q (a caller that splits its keypoints over several calls gets the
 * same rows):
 *   in-radius set   S = { i : d2(i) <= r2 }, in individually rounded fp32 (no fma): dx = p.x - q.x (dy, dz alike),
 *                   d2 = (dx*dx + dy*dy) + dz*dz, r2 = radius*radius; the comparison is inclusive, like
 *                   query_ball_point.  counts[q] = |S|, not clamped.
 *   key             key(i) = word0(Philox4x32-10(ctr_lo = i, ctr_hi = Q, key = seed)) >> (32 - key_bits)  -- the generator
 *                   of the dropout masks below; key_bits (1..32, production value 32) keeps only the top bits, so that a
 *                   test can force ties.
 *   count <= 1      idx row all -1, patch row all zeros (the reference returns a zero patch for len(indices) <= 1).
 *   count >= n_sample   the n_sample members of S smallest in (key, i) lexicographic order, written in ascending i: a
 *                   uniformly random subset without replacement that does not depend on how the work is scheduled.
 *   1 < count < n_sample   slots 0..count-1 hold S in ascending i; slot j >= count repeats slot
 *                   word1(Philox4x32-10(ctr_lo = j, ctr_hi = Q, key = seed)) mod count: a draw with replacement, with a
 *                   modulo bias of about count / 2^32.
 *   patches         (pc[idx] - center * kpt) * scale, center 0 or 1; the subtraction is rounded first, then the multiply.
 *                   With center = 0 and scale = 1 the values are bit copies of the fragment's.
 * 1 <= n, 0 <= k, 1 <= n_sample <= 8192, 1 <= key_bits <= 32, radius finite and > 0, center 0 or 1, no NULL pointer when
 * k > 0: EPN_EINVAL otherwise, decided before any HIP runtime call.  k == 0 succeeds and launches nothing.  One workgroup per
 * keypoint, no workspace, no global atomics: the result is bitwise repeatable. */
int epn_radius_patches_f32(const float *pc, int n, const float *kpts, int k, int64_t kpt_row0, float radius, int n_sample,
                           uint64_t seed, int key_bits, int center, float scale, int32_t *idx, int32_t *counts,
                           float *patches, epn_stream_t stream);

/* ModelNet training batches: a ragged set of raw clouds -> the [b, n_sample, 3] tensor, the rotations and the anchor labels
 * that the classification and rotation networks and their losses take.  Replaces the host path of the reference's ModelNet
 * loaders (SPConvNets/datasets/modelnet40.py:50-80 and :115-160), which per sample, in a DataLoader worker, resamples with
 * np.random.choice (pctk.uniform_resample_np, vgtk/vgtk/pc/sample.py:16-36), centres and scales (p3dtk.normalize_np,
 * vgtk/vgtk/point3d/normalize.py:30-34), rotates by scipy's Rotation.random (pctk.rotate_point_cloud,
 * vgtk/vgtk/pc/augmentation.py:58-89) and labels the rotation against the anchors (rotation_distance_np,
 * vgtk/vgtk/functional/rotation.py:350-369).  Those draws cannot be reproduced; this is the library's own deterministic form
 * of the same semantics (csrc/modelnet_batch.hip).
 *   points f32[m,3]: the clouds of a batch, concatenated; offsets i32[b+1] ON THE DEVICE: cloud c is rows offsets[c] ..
 *   offsets[c+1]-1, n_c of them; ids i64[b] on the device or NULL (id_c = c): the sample's identity, e.g. dataset index +
 *   epoch * dataset length.  With Q = id_c, every random draw of cloud c depends on (seed, Q) only -- never on c, on b or on
 *   the other clouds -- so a shuffled loader reproduces.
 *   -> pc_out f32[b,n_sample,3], pc_plain f32[b,n_sample,3] or NULL, idx i32[b,n_sample] (rows within the cloud), R f32[b,3,3],
 *      R_label i32[b], R_res f32[b,3,3], status i32[b]; every element is written on every call.
 *   selection     exactly the rule of epn_radius_patches_f32 with every point a member:
 *                 key(i) = word0(Philox4x32-10(ctr_lo = i, ctr_hi = Q, key = seed)) >> (32 - key_bits);
 *                 n_c >= n_sample: the n_sample indices smallest in (key, i), written in ascending i (n_c == n_sample is the
 *                 identity: the reference's test mode); 1 <= n_c < n_sample: slots 0..n_c-1 = 0..n_c-1 and slot j >= n_c is
 *                 word1(Philox4x32-10(ctr_lo = j, ctr_hi = Q, key = seed)) mod n_c.
 *   normalisation fp64 inside: c = the mean of the n_sample selected rows, duplicates counted (the reference normalises after
 *                 resampling); s = the largest |p - c| over them; p' = (p - c) / s.  pc_plain = p' rounded once.
 *   rotation      rot_mode 0: R = I.  rot_mode 2: R = R_in[c] (f32[b,3,3]: the reference's testR files).  rot_mode 1:
 *                 w = Philox4x32-10(ctr_lo = 2^32, ctr_hi = Q, key = seed), a counter no point index reaches;
 *                 u_k = (w[k] + 0.5) / 2^32, k = 0, 1, 2; Shoemake's quaternion x = sqrt(1-u0) sin(2 pi u1),
 *                 y = sqrt(1-u0) cos(2 pi u1), z = sqrt(u0) sin(2 pi u2), w = sqrt(u0) cos(2 pi u2); the standard
 *                 unit-quaternion matrix in fp64, rounded once to fp32: that fp32 matrix is R.
 *                 pc_out = R p' (the reference's convention, augmentation.py:87) in fp64 from the ROUNDED R, rounded once: the
 *                 returned R is exactly the rotation that was applied.
 *   anchor label  anchors f32[A,3,3], 1 <= A <= 64, or NULL (then R_label and R_res may be NULL and are not written).
 *                 R_label = arg max_i tr(A_i^T R) from the rounded R and the fp32 anchors, the nine products accumulated in fp64
 *                 in row-major order, the lowest i on a tie; R_res = A_label^T R in fp64, rounded once (the diff_r[label]
 *                 that the reference's flag == 'rotation' path trains on).
 *   status        bits 1, 2, 4, 8; the conditions exclude one another (a NaN extent is not == 0, an empty or badly delimited
 *                 cloud has no extent), so a cloud carries one of them, the first that applies: 8 offsets[c] > offsets[c+1] or outside [0, m]; 1 an empty
 *                 cloud; 4 a non-finite coordinate among the selected rows; 2 zero extent (s == 0; a one-point cloud is one);
 *                 0 otherwise.  A cloud with a status reads nothing out of range; its pc_out, pc_plain and R_res are zeros
 *                 and its idx is -1; its R is still drawn and its R_label computed.  Nothing asserts; no cloud affects another.
 * Refusals, decided before any HIP runtime call, all EPN_EINVAL: b < 0, m < 0, n_sample outside 1..8192, key_bits outside
 * 1..32, rot_mode outside 0..2, rot_mode 2 without R_in, anchors given with A outside 1..64; then b == 0 succeeds and launches
 * nothing; then a required pointer that is NULL (offsets, pc_out, idx, R, status; points when m > 0; R_label and R_res when
 * anchors is given).  One launch, one 256-thread workgroup per cloud, no workspace, no global atomics, no allocation, no host
 * synchronisation (the call can be captured into a HIP graph and replayed after ids were rewritten in place); the centroid is
 * summed in a fixed order: two calls are bitwise equal. */
int epn_modelnet_batch_f32(const float *points, int m, const int32_t *offsets, int b, const int64_t *ids, int n_sample,
                           uint64_t seed, int key_bits, int rot_mode, const float *R_in, const float *anchors, int A,
                           float *pc_out, float *pc_plain, int32_t *idx, float *R, int32_t *R_label, float *R_res,
                           int32_t *status, epn_stream_t stream);

/* 3DMatch training batches: a batch of fragment pairs with their keypoint correspondences -> the two patch tensors the
 * descriptor network trains on, the pair's relative rotation and the augmentation that was applied.  Replaces the host path of
 * the reference's FragmentLoader.__getitem__ (SPConvNets/datasets/match_3dmatch.py:301-354), which per pair, in a DataLoader
 * worker, draws npt correspondences with replacement (np.random.choice), cuts a radius patch around each keypoint in both
 * fragments (scipy KDTree), resamples every patch to input_num points (pctk.uniform_resample_np, vgtk/vgtk/pc/sample.py:16-36),
 * draws one Euler rotation per side (pctk.rotate_point_cloud(None, max_degree=30), vgtk/vgtk/pc/augmentation.py:16-33 and
 * :58-89), rotates the patches and returns T = R_A^T R_B.  Those draws cannot be reproduced; this is the library's own
 * deterministic form of the same semantics (csrc/pair_batch.hip).
 *   points f32[m,3], offsets i32[F+1] ON THE DEVICE: the F downsampled fragments of the batch, concatenated; fragment f is rows
 *   offsets[f] .. offsets[f+1]-1: the search support.  pairs i32[B,2]: the source and the target fragment of each sample, as rows
 *   of offsets; a fragment may serve several samples, source == target is allowed.  corr f32[C,2,3], corr_offsets i32[B+1]:
 *   sample b's keypoint correspondences are rows corr_offsets[b] .. corr_offsets[b+1]-1, P_b of them; entry [.,0] is a coordinate
 *   in the source fragment's frame and [.,1] in the target's (the reference takes them from the raw fragments).  poses f64[F,4,4]
 *   (row-major).  ids i64[B] on the device or NULL (id_b = b): the sample's identity, 0 <= id < 2^40, e.g. dataset index + epoch
 *   * dataset length.
 *   -> src, tgt f32[B,npt,n_sample,3], idx i32[B,2,npt,n_sample] (rows within the fragment), counts i32[B,2,npt],
 *      choice i32[B,npt], T f32[B,3,3], R_aug f32[B,2,3,3], T_aug f32[B,3,3], status i32[B]; every element is written on every call.
 * Every draw depends on (seed, id, npt) only -- never on b, on B or on the other samples.  The patch of sample id, side s
 * (0 source, 1 target), slot j has the stream Q' = (id * 2 + s) * npt + j.
 *   choice        choice[b,j] = word0(Philox4x32-10(ctr_lo = 2^32, ctr_hi = Q'(0,j), key = seed)) mod P_b: a draw with
 *                 replacement, at a counter no point index reaches; both sides use the same correspondence.
 *   patch         exactly the rule of epn_radius_patches_f32 applied to the rows of the side's fragment, with the keypoint
 *                 corr[choice[b,j], s] and the global row Q': the individually rounded fp32 distance, the inclusive comparison,
 *                 the (key, i) selection written in ascending i, the upsample draw and the count <= 1 zero row.  idx[b,s,j] and
 *                 counts[b,s,j] are bit for bit what that entry returns for the fragment alone with kpt_row0 = Q'.
 *   augmentation  side s: w = Philox4x32-10(ctr_lo = 2^32 + 1, ctr_hi = Q'(s,0), key = seed); degrees d_k = w[k] mod max_degree,
 *                 k = 0, 1, 2: integers in [0, max_degree) like np.random.randint(0, max_degree, 3), with a modulo bias of about
 *                 max_degree / 2^32; angles (d_k * pi) / 180; R = Rz(d_2) Ry(d_1) Rx(d_0) (R_from_euler_np) in fp64, rounded
 *                 once to fp32: that fp32 matrix is R_aug[b,s].  max_degree = 0: R = I (the reference's no_augmentation).
 *   values        R (p - center * q), center 0 or 1: the subtraction rounded in fp32 as in epn_radius_patches_f32, then each
 *                 component ((r0 x + r1 y) + r2 z) in fp64 from the ROUNDED R, rounded once: the returned R_aug is exactly the
 *                 rotation that was applied.  Zero rows stay zero.
 *   transforms    T = R_A^T R_B from the upper-left 3 x 3 blocks of poses[pairs[b,0]] and poses[pairs[b,1]], each entry
 *                 ((a0 b0 + a1 b1) + a2 b2) in fp64, rounded once (what the reference returns).  T_aug = (R_aug_src T) R_aug_tgt^T
 *                 from the three rounded matrices in fp64, rounded once: the relation the augmented patches satisfy (the reference
 *                 returns T although it hands rotated patches to the loss).
 *   status        a sample carries the first that applies: 8 a pairs entry outside [0,F), or offsets of one of its fragments or
 *                 its corr_offsets descending or outside [0,m] / [0,C]; 1 no correspondences; 4 a non-finite entry in one of its
 *                 two poses (all 16) or a non-finite coordinate in one of its npt chosen correspondences (either side); 0
 *                 otherwise.  A sample with a status reads nothing out of range; its src, tgt, T and T_aug are zeros, its idx and
 *                 choice -1, its counts 0; its R_aug is still drawn.  Nothing asserts; no sample affects another.  An empty patch
 *                 (also an empty fragment) is reported through counts, not through status.
 * Refusals, decided before any HIP runtime call, all EPN_EINVAL: B, F, m or C negative, n_sample outside 1..8192, npt outside
 * 1..4096, key_bits outside 1..32, max_degree outside 0..360, radius not finite or not > 0, center not 0 or 1, B * 2 * npt
 * beyond 2^31 - 1; then B == 0 succeeds and launches nothing; then a required pointer that is NULL (everything but ids; points
 * only when m > 0, corr only when C > 0, poses only when F > 0).  One launch of B * 2 * npt workgroups of 256 threads, each
 * doing what a workgroup of epn_radius_patches_f32 does and recomputing its sample's status and its side's R itself; no
 * workspace, no global atomics, no allocation, no host synchronisation (the call can be captured into a HIP graph and replayed
 * after ids were rewritten in place): two calls are bitwise equal. */
int epn_fragment_pair_batch_f32(const float *points, int m, const int32_t *offsets, int F, const int32_t *pairs, int B,
                                const float *corr, int C, const int32_t *corr_offsets, const double *poses, const int64_t *ids,
                                int n_sample, int npt, float radius, uint64_t seed, int key_bits, int max_degree, int center,
                                float *src, float *tgt, int32_t *idx, int32_t *counts, int32_t *choice, float *T, float *R_aug,
                                float *T_aug, int32_t *status, epn_stream_t stream);

/* Descriptor matching: for every fragment pair of a scene, the exact nearest neighbour in descriptor space in both
 * directions, then the mutual check "tgt -> src -> tgt", the ground-truth transform and the inlier count.  Replaces the host
 * block of the reference's evaluation (SPConvNets/datasets/evaluation_3dmatch.py:77-100: two sklearn KDTrees, the mutual
 * mask, hom_transform, distances < tau1); this is the library's own deterministic statement of it.
 *
 * Scene tables (shared by the two entries below and by epn_ransac_register_f64):
 *   frag_off i64[F+1]  row offsets of the fragments in the concatenated arrays: frag_off[0] = 0, ascending (an empty
 *                      fragment is allowed), frag_off[F] = R, fewer than 2^31 rows per fragment
 *   pairs    i32[P,2]  (src fragment, tgt fragment), both in 0..F-1, src != tgt, P <= 32767
 *   out_off  i64[P+1]  out_off[p] = sum over p' < p of n_src(p') + n_tgt(p'): pair p's block of the per-row outputs holds
 *                      its n_src src rows first, then its n_tgt tgt rows
 *   tgt_off  i64[P+1]  tgt_off[p] = sum over p' < p of n_tgt(p'): pair p's block of the per-tgt-row outputs
 * Every table is passed twice: `*_host` is read by the argument checks (on the host, before any HIP runtime call), the
 * unsuffixed pointer is the device copy the kernels read.  The caller computes out_off / tgt_off; the checks refuse tables
 * that do not follow the formulas.  The two copies must hold the same values.
 * Refusals: EPN_EINVAL for a size out of range, non-monotone offsets, a pair index out of range, src == tgt, or an offset
 * table off its formula; EPN_ENULL for a required pointer that is NULL; EPN_EWORKSPACE for a workspace that is NULL or too
 * small.  P == 0 (or no row at all) succeeds and launches nothing.
 *
 * epn_nn_match_f32 (replaces evaluation_3dmatch.py:77-84): feats f32[R,C], 1 <= C <= 128; valid u8[R] or NULL (all valid).
 *   For query row i of one fragment of a pair and every row j of the other:
 *     d2(i,j) = sum_c (a_ic - b_jc)^2, in fp32 FROM THE DIFFERENCES (never |a|^2 + |b|^2 - 2 a.b, which cancels twenty-fold
 *     for unit descriptors with a neighbour at d2 ~ 0.05); the order and fusion of the C additions are not specified.
 *     Row j is admissible iff it is valid and d2(i,j) is finite.
 *   nn_idx i32[out_off[P]]: the fragment-local index of the admissible row with the smallest d2, ties to the lowest index;
 *   nn_d2 f32[out_off[P]]: that d2.  An invalid query row, or one without an admissible candidate (a NaN row, an all-invalid
 *   or empty fragment on the other side), gets nn_idx = -1 and nn_d2 = +inf.  An invalid row is never chosen.
 *   Workspace: epn_nn_match_workspace_bytes(out_off[P]) bytes (host-only: 8 bytes per output row), 8-byte aligned.  The call
 *   sets it to all-ones with a memset on `stream`, combines the target segments with one 64-bit atomicMin per query on the
 *   key (bits(d2) << 32) | j, and unpacks it: the result does not depend on arrival order and is bitwise repeatable.
 *
 * epn_match_inliers_f64 (replaces evaluation_3dmatch.py:86-100): kp_xyz f32[R,3] keypoint coordinates in the row layout of
 *   feats; nn_idx as written above; gt f64[P,4,4] (row-major) takes tgt coordinates into src coordinates; tau1 not NaN.
 *   Tgt row j of pair p with s = nn_idx(tgt j) is mutual iff s >= 0 and nn_idx(src s) == j.  For a mutual row
 *     dist(j) = | kp_src[s] - (R kp_tgt[j] + t) |  in fp64 (R, t: the upper 3 x 4 of gt[p]),  inlier iff dist < tau1.
 *   match_src i32[tgt_off[P]] (s, or -1 if not mutual), match_dist f64[tgt_off[P]] (+inf if not mutual), n_match i32[P],
 *   n_inlier i32[P].  One workgroup per pair; the counts are an integer reduction inside it (no atomics).
 *   inlier_ratio = n_inlier / n_match is the host's (0 where n_match == 0; the reference divides by zero there). */
size_t epn_nn_match_workspace_bytes(int64_t out_rows);
int epn_nn_match_f32(const float *feats, int64_t R, int C, const uint8_t *valid, int F, const int64_t *frag_off_host,
                     const int64_t *frag_off, int P, const int32_t *pairs_host, const int32_t *pairs,
                     const int64_t *out_off_host, const int64_t *out_off, void *workspace, size_t workspace_bytes,
                     int32_t *nn_idx, float *nn_d2, epn_stream_t stream);
int epn_match_inliers_f64(const float *kp_xyz, int64_t R, int F, const int64_t *frag_off_host, const int64_t *frag_off, int P,
                          const int32_t *pairs_host, const int32_t *pairs, const int64_t *out_off_host, const int64_t *out_off,
                          const int64_t *tgt_off_host, const int64_t *tgt_off, const int32_t *nn_idx, const double *gt,
                          double tau1, int32_t *match_src, double *match_dist, int32_t *n_match, int32_t *n_inlier,
                          epn_stream_t stream);

/* Pairwise registration: the rigid transform between the two fragments of every pair of a scene from its mutual matches alone,
 * by hypothesise-and-verify (RANSAC) over three-point samples and one least-squares refit.  No ground truth
 * enters.  The reference stops at feature-match recall; the host tool usually run for this step is open3d's
 * registration_ransac_based_on_feature_matching.  This is the library's own deterministic statement of it.
 *
 * epn_ransac_register_f64: the scene tables frag_off, pairs and tgt_off of the matching entries above (host and device copy
 *   each, the same refusal rules); kp_xyz f32[R,3]; match_src i32[tgt_off[P]] as epn_match_inliers_f64 writes it (-1 = not
 *   mutual); tau f64, finite and > 0; H hypotheses per pair, 1 <= H <= 65536; seed u64; pair0 >= 0, the counter word of
 *   pairs[0] (pair p of the call draws as pair pair0 + p, so a pair gives the same result alone and in a batch);
 *   min_margin f64, 0 <= min_margin < 1.
 *   Correspondences of pair p: its tgt rows j with 0 <= s = match_src[j] < n_src(p), numbered m = 0..M_p-1 in ascending j;
 *     x_m = kp_src[s], y_m = kp_tgt[j], widened to fp64.  match_src is range-checked on the device: an entry >= n_src(p) is
 *     dropped like a negative one and never used as an index.
 *   Draw: hypothesis h takes i_k = word_k(Philox4x32-10(ctr_lo = h, ctr_hi = pair0 + p, key = seed)) mod M_p, k = 0, 1, 2 (a
 *     modulo bias of about M_p / 2^32, as in epn_radius_patches_f32).  It is REJECTED if M_p < 3 or two i_k are equal.
 *   Fit of a set S (Horn), fp64: centroids xbar, ybar over S; C = sum_{m in S} (x_m - xbar)(y_m - ybar)^T; (R, margin) = the
 *     projection of epn_so3_mean_f32 above applied to C (R maximises tr(R^T C), margin = (s2 + d s3) / s1); t = xbar - R ybar.
 *     (R, t) takes tgt coordinates into src coordinates, the direction of gt in epn_match_inliers_f64.  A hypothesis whose
 *     three-point fit has margin < min_margin is rejected too (collinear or coincident samples have margin 0).
 *   Score: count[h] = #{m : |x_m - (R y_m + t)|^2 < tau^2} in fp64 over all M_p correspondences; -1 for a rejected hypothesis.
 *   Choice: best_h = the h with the largest count, the lowest h on a tie.  The pair FAILS if count[best_h] < 3 (which includes
 *     every hypothesis rejected): T = I, best_h = -1, n_inlier = 0, rmse = +inf, margin = 0.
 *   Refit: one fit over the inlier set of best_h.  That fit is the result; its margin is reported, not tested (always a
 *     rotation, conditioning reported, as epn_so3_mean_f32).  n_inlier and rmse = sqrt(mean of the squared inlier distances)
 *     are taken again under the refitted transform; rmse = +inf when that set is empty.
 *   Outputs: T f64[P,4,4] row-major with bottom row 0 0 0 1; best_h i32[P]; hyp_count i32[P,H], every hypothesis' score (an
 *     output, not scratch: it is what makes the entry testable); n_inlier i32[P]; rmse f64[P]; margin f64[P].
 *   Workspace: epn_ransac_register_workspace_bytes(tgt_off[P]) bytes (host-only: 24 bytes per tgt row for the compacted
 *     correspondences, rounded up to 8, plus 4 bytes for each of the 32768 pair counts), 8-byte aligned; written by the call.
 *   Three launches (compact, score, finish: csrc/ransac_register.hip); no atomics; the refit's sums run in a fixed order
 *   (thread i adds m = i, i + 256, ... ascending, then a fixed tree), so two runs are bitwise equal.  Every loop is bounded by
 *   a row count, M_p, H or the projection's sweep count.
 *   Refusals, decided before any HIP runtime call: EPN_EINVAL for H, tau, min_margin or pair0 out of range (NaN included), then
 *   the scene-table refusals; P == 0 succeeds and launches nothing; then EPN_ENULL for a required pointer that is NULL
 *   (kp_xyz and match_src only if there is a tgt row), EPN_EWORKSPACE for a workspace that is NULL or too small. */
size_t epn_ransac_register_workspace_bytes(int64_t tgt_rows);
int epn_ransac_register_f64(const float *kp_xyz, int64_t R, int F, const int64_t *frag_off_host, const int64_t *frag_off, int P,
                            const int32_t *pairs_host, const int32_t *pairs, const int64_t *tgt_off_host, const int64_t *tgt_off,
                            const int32_t *match_src, double tau, int H, uint64_t seed, int64_t pair0, double min_margin,
                            void *workspace, size_t workspace_bytes, double *T, int32_t *best_h, int32_t *hyp_count,
                            int32_t *n_inlier, double *rmse, double *margin, epn_stream_t stream);

/* Voxel-grid downsampling: one centroid per occupied voxel of ONE fragment.  The reference never searches the raw fragment:
 * radius_ball_search_o3d (SPConvNets/datasets/match_3dmatch.py:107-139) calls open3d's pcd.voxel_down_sample(voxel_size)
 * first (0.03 below 1024 input points, 0.015 from there: :258, :371, :445) and builds its KD-tree over the centroids.  This is
 * open3d's VoxelDownSample made deterministic; it has not been run against open3d.
 *   pc f32[n,3] (row-major), voxel_size (a double, as in open3d) -> centroids f32[M,3], counts i32[M], first_idx i32[M],
 *   point_voxel i32[n], status i32[2] = {M, flags} on the device.  The caller allocates n rows for the per-voxel outputs.
 *   dropped points  a point with any non-finite coordinate takes no part in anything below; its point_voxel entry is -1.
 *   voxel index     lo = per-axis minimum over the kept points (an fp32 minimum: exact, independent of order).  In fp64:
 *                   vmin = (double)lo - 0.5 * voxel_size,  ix = floor(((double)x - vmin) / voxel_size)  (iy, iz alike) --
 *                   open3d's voxel_min_bound and floor(ref_coord).  key = ix << 42 | iy << 21 | iz.
 *   range errors    flags bit 0: a kept |coordinate| > 256; bit 1: an index >= 2^21; (bit 2: the table overflowed, which the
 *                   load factor below excludes).  With flags != 0 nothing else in the outputs is defined; nothing is
 *                   dropped silently.
 *   centroid        per coordinate fx = llrint((double)x * 2^32) (exact for |x| >= 2^-9), summed as 64-bit integers over the
 *                   voxel's points (256 * 2^32 * 2^22 < 2^63), so the sum does not depend on order and is bitwise repeatable;
 *                   centroid = (float)((double)sum / ((double)count * 2^32)).
 *   output order    voxels in ascending order of their lowest member point index (open3d's order is its hash map's);
 *                   first_idx holds that index, point_voxel the output row of each kept point's voxel.  The rows are ranked
 *                   by a prefix sum over "first point of its voxel" flags in tiles of 256 points: per-tile counts, one
 *                   workgroup that scans the counts 256 at a time, the write pass.
 * Hash table (stated because tests construct collisions from it): open addressing in the caller's workspace, capacity the
 * smallest power of two >= max(2n, 128), an empty slot's key all-ones (no valid key has bit 63 set), home slot
 * (key * 0x9E3779B97F4A7C15) >> (64 - log2(capacity)) in 64-bit wrapping arithmetic, probed linearly with wrap-around.
 * Workspace: epn_voxel_downsample_workspace_bytes(n) bytes (host-only), 8-byte aligned; initialised by the call itself.
 * 0 <= n <= 2^22, voxel_size finite and > 0, no NULL pointer and a large enough workspace when n > 0: EPN_EINVAL otherwise,
 * decided before any HIP runtime call.  n == 0 succeeds, launches nothing and leaves status untouched. */
size_t epn_voxel_downsample_workspace_bytes(int64_t n);
int epn_voxel_downsample_f32(const float *pc, int64_t n, double voxel_size, float *centroids, int32_t *counts,
                             int32_t *first_idx, int32_t *point_voxel, int32_t *status, void *workspace,
                             size_t workspace_bytes, epn_stream_t stream);

/* Point grid: the nearest point of ONE cloud within a bound, for 3-D queries (csrc/point_grid.hip).  It is the one
 * primitive of the reference's keypoint stage (SPConvNets/datasets/preprocess/run_keypoint.py), which runs it on the host:
 * sklearn's NearestNeighbors in test_scenes_overlap (:98-112), in cross_filtering_via_fpfh (:30-37, :66-67) and in the map back to
 * raw rows (:131-138), and open3d's radius search behind compute_fpfh_feature (:47-48), of which only "is there another point
 * within the radius" survives (:58-59).
 *
 * epn_point_grid_build_f32: ref f32[n,3] (row-major), ref_valid u8[n] or NULL, max_radius -> the grid, in the caller's workspace,
 *   and status i32[2] = {kept, flags} on the device.
 *   participation   a reference point takes part when all three coordinates are finite and ref_valid is NULL or its byte is
 *                   non-zero.  kept = the number of points in the grid.
 *   cell            edge = max_radius * (1 + 2^-10) in fp64.  Index, key, hash table and range flags are exactly
 *                   epn_voxel_downsample_f32's with voxel_size = edge and "kept" read as "participating": lo = per-axis fp32
 *                   minimum, ix = floor(((double)x - ((double)lo - 0.5 * edge)) / edge), key = ix << 42 | iy << 21 | iz,
 *                   capacity the smallest power of two >= max(2n, 128), home slot (key * 0x9E3779B97F4A7C15) >> (64 -
 *                   log2(capacity)), linear probing with wrap-around; flags bit 0: a participating |coordinate| > 256, bit 1: an
 *                   index >= 2^21 (bit 2: the table overflowed, which the load factor excludes).  With flags != 0 the grid is
 *                   not to be queried (such points are left out of it; a query stays inside the workspace all the same).
 *   records         the points are counting-sorted by cell into 16-byte records {x, y, z, row}: per-cell counts (integer
 *                   atomics), one scan over the table's slots (per-tile sums of 256 slots, one workgroup that scans the sums 256
 *                   at a time, the offsets), a scatter through returned integer atomicAdd cursors.  The order of the records
 *                   inside a cell is free and no output of either entry depends on it; the workspace's bytes are not part of
 *                   the contract.
 *   Why 27 cells suffice: let p be admissible for a query q, that is d2 <= r2 below with radius <= max_radius, and take one axis.
 *     fl(dx * dx) <= d2 (adding non-negative terms and rounding never goes below a representable term), r2 <= radius^2 (1 +
 *     2^-24), and fl(dx * dx) >= (p - q)^2 (1 - 2^-24)^3 unless it underflows, which needs |p - q| < 2^-63 (hence max_radius >=
 *     2^-60).  So |p - q| <= max_radius (1 + 2^-22) <= edge (1 - 2^-11): the exact quotients (x - vmin) / edge of p and q differ by
 *     less than 1 - 2^-11.  The computed ones are each within 2^21 * 2^-51 = 2^-30 of the exact ones (two fp64 roundings on a
 *     value below 2^21; vmin is the same fp64 number for both), so they differ by less than 1 and their floors by at most 1.
 *   Workspace: epn_point_grid_workspace_bytes(n) bytes (host-only; 0 outside 0 <= n <= 2^22), 16-byte aligned; initialised by
 *   the call itself.  Seven launches; nothing depends on arrival order but the order inside a cell.
 *   0 <= n <= 2^22, max_radius finite and >= 2^-60, a large enough workspace, and ref and status when n > 0: EPN_EINVAL
 *   otherwise, decided before any HIP runtime call.  n == 0 builds an empty grid: it launches nothing, leaves status untouched,
 *   and every query on it answers -1.
 *
 * epn_point_grid_nn_f32: the grid of a build (the same workspace address and n), qry f32[m,3], radius -> nn_idx i32[m],
 *   nn_d2 f32[m], hits i32[1] or NULL.
 *   answer          among the points of the grid with d2 <= r2, the one with the smallest d2, on a tie the lowest row:
 *                   nn_idx = its row in ref, nn_d2 = its d2; -1 and +inf when there is none.
 *                   d2 = (dx*dx + dy*dy) + dz*dz, dx = p.x - q.x, every operation individually rounded in fp32 (no fma), as
 *                   epn_radius_patches_f32's membership test; r2 = (float)(radius * radius), the product taken in fp64.
 *   exclude_row     1: the candidate whose row equals the query's own index is skipped (a cloud searched against itself, m == n
 *                   required; a duplicate of the point at another row is still found, with d2 = 0).  0: nothing is skipped.
 *   no answer       a query with a non-finite coordinate reads no cell and gets -1.  A cell whose index is outside [0, 2^21) on
 *                   an axis holds no point and is not looked up, so a query far outside the cloud gets -1 as well.
 *   hits            the number of queries with nn_idx >= 0: zeroed on the stream by a one-wave launch of the library's own (no
 *                   memset), then one integer atomicAdd per workgroup of the query.
 *   One wave per query, four per workgroup: lanes 0..26 look up the 27 cells, the wave strides over their records with 16-byte
 *   loads, and the best (d2 bits << 32 | row, one 64-bit key: d2 >= 0, so its bits order like its value) is the minimum over the
 *   wave.  Integer minima and sums only: two runs are bitwise equal.  No host synchronisation: build and query can be captured
 *   into a HIP graph on one stream.
 *   The library remembers (n, max_radius) of the last build per workspace address on the host (at most 2^16 addresses; when a
 *   build would exceed that, the older entries are forgotten and their grids must be built again).
 *   0 <= n, m <= 2^22, radius finite, 0 < radius <= max_radius of the build, exclude_row 0 or 1 and m == n with 1, a workspace
 *   address and n that a build has been called with, and qry, nn_idx, nn_d2 when m > 0: EPN_EINVAL otherwise, decided before any
 *   HIP runtime call.  m == 0 succeeds (hits, if given, becomes 0). */
size_t epn_point_grid_workspace_bytes(int64_t n);
int epn_point_grid_build_f32(const float *ref, int64_t n, const uint8_t *ref_valid, double max_radius, void *workspace,
                             size_t workspace_bytes, int32_t *status, epn_stream_t stream);
int epn_point_grid_nn_f32(const void *workspace, int64_t n, const float *qry, int64_t m, double radius, int exclude_row,
                          int32_t *nn_idx, float *nn_d2, int32_t *hits, epn_stream_t stream);

/* Surface normals and patch frames (csrc/point_normals.hip, csrc/plane_fit.h): the reference's --normals switch
 * (opt.model.normals).  It estimates a fragment's normals once on the host with open3d (preprocess/run_fusion.py:48,
 * pc.estimate_normals()), reads them at the keypoints (match_3dmatch.py:117-120) and turns every patch into its keypoint's normal
 * frame (transform_with_normals, :141-152).  The contract fixes the result, not the schedule.
 *
 * epn_point_normals_f32: the grid of a build (workspace address and n, as epn_point_grid_nn_f32 takes them), qry f32[m,3], radius,
 *   max_nn, view f32[3] on the device or NULL -> normals f32[m,3], eig f32[m,3], count i32[m], flags i32[m], and, each NULL-able,
 *   moments i64[m,9] and nbr_idx i32[m,max_nn].
 *   in-radius set   the grid's points with d2 <= r2, d2 and r2 exactly as in epn_point_grid_nn_f32 (individually rounded fp32, no
 *                   fma, inclusive, r2 = (float)(radius * radius) from the fp64 product).  The query's own point, when it is in
 *                   the grid, is a member like any other.  count = the size of this set, not clamped.
 *   neighbourhood   max_nn > 0 and count > max_nn: the max_nn members smallest in the 64-bit key d2 bits << 32 | row, which is
 *                   open3d's KDTreeSearchParamHybrid made deterministic (the lowest row on a distance tie).  Otherwise the whole
 *                   set (KDTreeSearchParamRadius).  used = min(count, max_nn) (= count with max_nn == 0).  nbr_idx holds the
 *                   neighbourhood's rows in ascending key order, -1 beyond used.
 *   moments         for a neighbour p of the query q, per axis t = ((double)p - (double)q) / radius: two fp64 operations, each
 *                   rounded once.  S_i = sum rint(t_i 2^40), M_ij = sum rint((t_i t_j) 2^40) for ij = xx, xy, xz, yy, yz, zz, the
 *                   product rounded once (no fma) before the exact scaling; all sums int64.  |t| < 1 + 2^-20 and n <= 2^22 keep
 *                   every sum below 2^63.  moments = {S_x, S_y, S_z, M_xx, M_xy, M_xz, M_yy, M_yz, M_zz}.  Integer sums do not
 *                   depend on their order, and the order of the records inside a cell is free: hence the fixed point.
 *   plane fit       in fp64, every operation rounded on its own: mean_i = (S_i / 2^40) / used, C_ij = (M_ij / 2^40) / used -
 *                   mean_i mean_j; a cyclic Jacobi (10 sweeps over (0,1), (0,2), (1,2), the rotations of the SO(3) projection)
 *                   gives the eigenvalues, sorted ascending with the lowest index first on a tie; eig = (float)(lambda * (radius *
 *                   radius)); the normal is the eigenvector of lambda0, normalised in fp64.
 *   sign            with view: flipped so that (n0 (v0 - q0) + n1 (v1 - q1)) + n2 (v2 - q2) >= 0 in fp64 (open3d's
 *                   orient_normals_towards_camera_location; a fused fragment's own origin is a camera position).  Without: the
 *                   component of largest magnitude is positive, the lowest axis on a tie.  Then rounded once to fp32.
 *   flags           bit 0: used < 3; the normal is (0, 0, 1), whatever the view, and eig is zero (open3d's fallback).  bit 1: a
 *                   non-finite query coordinate; it reads no cell, count = 0 (so bit 0 is set as well).  bit 2: lambda1 -
 *                   lambda0 <= 2^-40 in the units of C: the direction is not determined; the computed one is still returned.
 *                   Nothing asserts, and no query affects another.
 *   self_rows       1 states that the queries are the grid's own points (m == n is required); nothing is skipped.
 *   One launch: one wave per query, four per workgroup; count, a bisection on the key for the max_nn cut (only where count >
 *   max_nn), the moment sweep with an integer xor tree across the wave, then threads 0..3 of the workgroup finish one query each.
 *   No floating-point atomics, no allocation, no host synchronisation: bitwise repeatable and graph-capturable.
 *   0 <= n, m <= 2^22, radius finite, 0 < radius <= max_radius of the build, max_nn in 0..1024, no nbr_idx with max_nn == 0,
 *   self_rows 0 or 1 and m == n with 1, a workspace address and n that a build has been called with, and qry, normals, eig, count,
 *   flags when m > 0: EPN_EINVAL otherwise, decided before any HIP runtime call.  m == 0 succeeds and launches nothing.
 *
 * epn_orient_patches_f32: patches f32[k,n_sample,3], normals f32[k,3] -> axis f32[k,3,3], out f32[k,n_sample,3]; out may be
 *   patches.  u(v) = v / (|v| + 1e-5) with |v| = sqrt((v0 v0 + v1 v1) + v2 v2), all in fp64, every operation rounded on its own:
 *   z = u(n), x = u(up cross z) with up = (0, -1, 0), y = u(z cross x), the cross product (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 -
 *   a1 b0); axis has x, y, z as its COLUMNS, rounded once to fp32.  With the normal parallel to up the frame's x and y are zero,
 *   as upstream; nothing becomes NaN.  out = patch @ axis: component j = ((p0 a0j + p1 a1j) + p2 a2j) in fp64 from the ROUNDED
 *   axis, rounded once (the convention of epn_fragment_pair_batch_f32's rotation); zero rows stay zero.  One workgroup per patch,
 *   one launch.  0 <= k <= 2^22, n_sample in 1..8192, no NULL pointer when k > 0: EPN_EINVAL otherwise, decided before any HIP
 *   runtime call.  k == 0 succeeds and launches nothing. */
int epn_point_normals_f32(const void *workspace, int64_t n, const float *qry, int64_t m, double radius, int max_nn, int self_rows,
                          const float *view, float *normals, float *eig, int32_t *count, int32_t *flags, int64_t *moments,
                          int32_t *nbr_idx, epn_stream_t stream);
int epn_orient_patches_f32(const float *patches, const float *normals, int64_t k, int n_sample, float *axis, float *out,
                           epn_stream_t stream);

/* FPFH descriptors (csrc/fpfh.hip, csrc/fpfh_math.h): the reference's compute_fpfh_feature
 * (SPConvNets/datasets/preprocess/run_keypoint.py:40-50), which runs open3d's compute_fpfh_feature with KDTreeSearchParamRadius on
 * the host.  The steps are open3d's ComputePairFeatures, ComputeSPFHFeature and ComputeFPFHFeature, made independent of the
 * order of the neighbours.  It is argued from open3d's algorithm, not run against it: open3d is not installed where this was
 * written.  The numpy restatement (tests/fpfh_ref.py) is the contract; it fixes the result, not the schedule.
 *
 * epn_point_fpfh_f32: the grid of a build (grid_workspace and n, as epn_point_grid_nn_f32 takes them), points f32[n,3] = the
 *   cloud the grid was built from, normals f32[n,3], radius -> fpfh f32[n,33] row-major (open3d's .data.T), count i32[n],
 *   flags i32[n] and, NULL-able, spfh i32[n,33].  The queries are always the grid's own points: a pair feature needs the query's
 *   normal, so there is no foreign-query form.
 *   neighbourhood   of point i: the grid's points k != i (by row) with d2 <= r2, d2 and r2 exactly as in epn_point_grid_nn_f32
 *                   (individually rounded fp32, no fma, inclusive, r2 = (float)(radius * radius) from the fp64 product).  d2 is
 *                   symmetric, so k is a neighbour of i exactly when i is one of k.  A duplicate at another row is a neighbour
 *                   (d2 = 0).  used = the size of this set = count.  Radius search only (KDTreeSearchParamRadius, the
 *                   reference's call); open3d's hybrid max_nn cut is not offered.
 *   pair features   of (i, k), all in fp64 on the promoted fp32 inputs, every operation rounded on its own (no fma), dot products
 *                   as (a0 b0 + a1 b1) + a2 b2, cross products as (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0):
 *                   d = p_k - p_i, len = sqrt(d . d); len == 0: f = (0, 0, 0).  a1 = (n_i . d) / len, a2 = (n_k . d) / len.
 *                   |a1| < |a2| (open3d: acos(|a1|) > acos(|a2|); the two differ only where acos rounds two arguments to one
 *                   value, or for |a| > 1): n1 = n_k, n2 = n_i, d = -d, f3 = -a2; otherwise n1 = n_i, n2 = n_k, f3 = a1.
 *                   v = d x n1; |v| == 0: f = (0, 0, 0); else v = v / |v|, w = n1 x v, f2 = v . n2, f1 = atan2(w . n2, n1 . n2)
 *                   with a first argument of -0 taken as +0.  A normal (of i or of k) with a non-finite component: f = (0, 0, 0).
 *   bins            h1 = floor((11 (f1 + pi)) / (2 pi)), h2 = floor((11 (f2 + 1)) 0.5), h3 = floor((11 (f3 + 1)) 0.5), each
 *                   clamped to 0..10.  Every neighbour adds 1 to c_i(h1), c_i(11 + h2), c_i(22 + h3): spfh = c_i, integers.
 *                   open3d's SPFH is 100 c_i(j) / used_i, which it reaches by adding 100 / used per neighbour in floating point.
 *   fpfh            d2min = the smallest non-zero d2_k over the neighbours of i.  For every neighbour k with d2_k > 0,
 *                   term_k(j) = rint(((d2min / d2_k) (c_k(j) / used_k)) 2^40): the two quotients and the product rounded once
 *                   each, the scaling exact.  A(j) = sum_k term_k(j) and G(g) = the sum of A over the eleven bins of group g,
 *                   both int64: integer sums do not depend on their order.  fpfh(j) = (float)((100 A(j)) / G(g) +
 *                   (100 c_i(j)) / used_i), the first quotient 0 when G(g) == 0.  This is open3d's FPFH with its two deviations
 *                   from the paper (the weight is 1 / d2, not 1 / d; the point's own SPFH is added after the normalisation to
 *                   100); the common factor d2min cancels in A / G and is there to bound the terms: term <= 2^40, the eleven
 *                   terms of one neighbour and group add up to at most 2^40 + 11, and n <= 2^22 keeps A and G below 2^63.
 *   flags           bit 0: used == 0; the row is zero.  bit 1: a non-finite coordinate or normal component of the point, or a
 *                   point the grid leaves out (ref_valid); the rows of fpfh and spfh are zero.  A point the grid leaves out is
 *                   nobody's neighbour and has count = 0 (so bit 0 is set as well); a point in the grid whose normal is not
 *                   finite keeps its count, stays a neighbour, and adds the features (0, 0, 0) to its neighbours' counts and
 *                   nothing to their weighted sums.  Nothing asserts, and no point affects another beyond this.
 *   Two launches, one wave per point and four per workgroup in both: the counts (per-wave integer histograms in LDS), then the
 *   weighted sums (one bin per lane, one int64 each).  No floating-point atomics, no allocation, no host synchronisation: bitwise
 *   repeatable and graph-capturable.
 *   Workspace: epn_point_fpfh_workspace_bytes(n) bytes (host-only; 0 outside 0 <= n <= 2^22), 16-byte aligned, written by the
 *   first launch: c i32[n,33] and d2min f32[n].
 *   0 <= n <= 2^22, radius finite, 0 < radius <= max_radius of the build, a grid workspace address and n that a build has been
 *   called with, and, when n > 0, points, normals, fpfh, count, flags and a large enough workspace: EPN_EINVAL otherwise, decided
 *   before any HIP runtime call.  n == 0 succeeds and launches nothing. */
size_t epn_point_fpfh_workspace_bytes(int64_t n);
int epn_point_fpfh_f32(const void *grid_workspace, int64_t n, const float *points, const float *normals, double radius, float *fpfh,
                       int32_t *count, int32_t *flags, int32_t *spfh, void *workspace, size_t workspace_bytes,
                       epn_stream_t stream);

/* ICP refinement: the dense alignment after epn_ransac_register_f64 (csrc/icp_refine.hip, csrc/icp_math.h).  This
 * is open3d's registration_icp with TransformationEstimationPointToPoint or TransformationEstimationPointToPlane and
 * ICPConvergenceCriteria(relative_fitness, relative_rmse, max_iteration), made deterministic.  It is argued from open3d's
 * algorithm; open3d is not installed where this was written, and the stage has not been run against it.  The contract fixes the
 * result, not the schedule.
 *
 * epn_icp_refine_f32: the target's grid (grid_workspace and n, as epn_point_grid_nn_f32 takes them), tgt_normals f32[n,3] or NULL
 *   (NULL: point-to-point; otherwise point-to-plane), src f32[m,3], T_init f64[4,4] row-major taking src into the target's frame
 *   (only its first three rows are read), max_dist, max_iter, rel_fitness, rel_rmse -> all on the device: T f64[4,4] (bottom row
 *   written 0 0 0 1; T may be T_init), trace f64[max_iter,20], iterations i32[1], status i32[1], and, each NULL-able, sums i64[32]
 *   and nn_idx i32[m].
 *   Iteration k = 0 .. max_iter-1 starts from T_k (T_0 = T_init) and does, in this order:
 *   transform     q_i = (float)fma(T_i0, s_0, fma(T_i1, s_1, fma(T_i2, s_2, T_i3))) for every source point s, the fp32
 *                 coordinates widened to fp64: three explicit fp64 fmas per component (the chain of csrc/rigid_fit.h's
 *                 sq_residual), rounded once to fp32.
 *   correspond    the answer of epn_point_grid_nn_f32 for the query q with radius = max_dist and exclude_row = 0: individually
 *                 rounded fp32 d2, r2 = (float)(max_dist * max_dist), inclusive, the lowest row on a tie, only the points that
 *                 took part in the build (its ref_valid mask), nothing for a non-finite or far q.  p = that point, as fp32.
 *   range         a matched pair is OUT OF RANGE when not |p_i| <= 64 and |q_i| <= 64 on every axis (NaN counts), and in
 *                 point-to-plane mode when not |n_i| <= 1 for every component of the normal n = tgt_normals[row of p].  Such a
 *                 pair adds to no sum below; it is counted in sum 30, and any such pair raises flag bit 3 (below).
 *   accumulate    every other matched pair adds one term to each int64 sum of a row of 32.  All values are fp64, every
 *                 operation rounded on its own (no fma); d = q - p per axis, dd = (d0 d0 + d1 d1) + d2 d2.  A term is
 *                 rint((a b) * scale), the product rounded once before the exact power-of-two scaling, ties to even (the rule
 *                 of epn_point_normals_f32's moments).  Origin: the coordinate origin of the target's frame.  Quanta: 2^-32 for
 *                 the linear sums, 2^-24 for the product sums.
 *                   point-to-point   [0] count; [1..3] p_i 2^32; [4..6] q_i 2^32; [7 + 3i + j] (p_i q_j) 2^24; [16] dd 2^24.
 *                   point-to-plane   c = q x n (c0 = q1 n2 - q2 n1, c1 = q2 n0 - q0 n2, c2 = q0 n1 - q1 n0), r = (d0 n0 + d1 n1) +
 *                                    d2 n2, J = (c0, c1, c2, n0, n1, n2).  [0] count; [1..21] (J_i J_j) 2^24 for i <= j, row-major
 *                                    (00, 01, .., 05, 11, ..); [22 + i] (J_i r) 2^24; [28] (r r) 2^24; [29] dd 2^24.
 *                 [30] = the number of out-of-range pairs; the other entries are 0.
 *                 Why no sum leaves int64: in range, |p_i|, |q_i| <= 2^6 and |n_i| <= 1 give |c_i| <= 2^7, |d_i| <= 2^7, |r| <= 3 *
 *                 2^7, so every product is at most r r <= 9 * 2^14 < 2^18 (p_i q_j <= 2^12, dd <= 3 * 2^14, J_i r <= 3 * 2^14) up to
 *                 rounding, a product term at most 2^42 + 1 and a linear term at most 2^38; with m <= 2^20 points every sum is
 *                 below 2^62 + 2^20 < 2^63.  Hence m <= 2^20 (EPN_EINVAL beyond, decided on the host) and the range +-64.
 *                 (2^18 pads the largest product, 9 * 2^14: by the unpadded figure 2^21 points would still fit, 9 * 2^59 < 2^63,
 *                 and 2^22 would not.  The limit refused beyond is the padded bound's 2^20: one bit of slack, stated, not used.)
 *   step          N = count, ssd = [dd sum] / 2^24, rmse = sqrt(ssd / N) (0 when N = 0: open3d's inlier_rmse is the Euclidean one
 *                 in both variants), fitness = N / m.  The first that applies, flag bits in brackets:
 *                   [3] an out-of-range pair;
 *                   [1] N < 3 (point-to-point) or N < 6 (point-to-plane);
 *                   [0] k > 0 and |fitness_k - fitness_{k-1}| < rel_fitness and |rmse_k - rmse_{k-1}| < rel_rmse: open3d's test,
 *                       which compares two successive evaluations; this is "converged", not a failure;
 *                   [2] the solve below is singular;
 *                   otherwise T_{k+1} = dT T_k, no flag.
 *                 With any flag T_{k+1} = T_k and the loop STOPS: every later iteration is a no-op whose trace record repeats this
 *                 one.  iterations = the number of iterations that updated T (open3d's loop count when it breaks); status = the OR
 *                 of the flags met (0: max_iter updates were made without the stop test being met).
 *   solve, point-to-point   sp = S_p / 2^32, sq = S_q / 2^32, pbar = sp / N, qbar = sq / N, C_ij = S_pq,ij / 2^24 - (sp_i sq_j) / N;
 *                 (dR, margin) = the projection of epn_so3_mean_f32 applied to C, dt = pbar - dR qbar (csrc/rigid_fit.h's
 *                 fit_finish, the fit of epn_ransac_register_f64).  Singular: not margin > 1e-6.
 *   solve, point-to-plane   A = the symmetric 6 x 6 of sums [1..21] / 2^24, b = sums [22..27] / 2^24.  A = L D L^T without pivoting,
 *                 k ascending: d_k = A_kk - sum_{j<k} (L_kj d_j) L_kj, L_ik = (A_ik - sum_{j<k} (L_ij d_j) L_kj) / d_k, sums from the
 *                 left in ascending j.  Singular: not d_k > 2^-20 A_kk for some k (all normals parallel, a single plane, ...), or
 *                 a non-finite solution.  L y = -b (ascending), z = y / d, L^T x = z (descending); w = x[0..3), dt = x[3..6).
 *                 dR = the Cayley map (I - [w]x / 2)^-1 (I + [w]x / 2) in closed form: a = w / 2, aa = (a0 a0 + a1 a1) + a2 a2,
 *                 k = 1 - aa, den = 1 + aa, dR_ii = (k + w_i a_i) / den, dR_01 = (w0 a1 - w2) / den, dR_02 = (w0 a2 + w1) / den,
 *                 dR_10 = (w1 a0 + w2) / den, dR_12 = (w1 a2 - w0) / den, dR_20 = (w2 a0 - w1) / den, dR_21 = (w2 a1 + w0) / den.
 *                 This is the ONE deliberate difference from open3d, which composes the Euler rotations Rz(w2) Ry(w1) Rx(w0):
 *                 the Cayley map needs + - x / only, is an exact rotation for every w, agrees with open3d's to second order in w
 *                 and has the same fixed point (w = 0), so a restatement follows it without a libm in the way.
 *   compose       rows 0..2: T'_ij = (dR_i0 T_0j + dR_i1 T_1j) + dR_i2 T_2j, and then T'_i3 += dt_i.
 *   All of "step" is fp64 with every operation rounded on its own, except inside the projection, which is compiled as it is
 *   for epn_ransac_register_f64; so T is reproducible bit for bit between runs, and a restatement (tests/icp_ref.py) meets it
 *   within a bound, while correspondences, counts and sums are integers and are met exactly.
 *   trace         record k = {T_{k+1} (16), N, ssd, rmse, flags} of iteration k, as doubles.  The count and rmse of a record are
 *                 those of T_k, the transform the iteration STARTED from: max_iter iterations make max_iter searches, where
 *                 open3d makes one more to evaluate its final transform.  After a stop the last live record's N and rmse ARE those
 *                 of the final T.  sums and nn_idx are those of the last live iteration (nn_idx: the row of p, or -1).
 *   Degenerate sizes: m == 0 or max_iter == 0 succeeds with T = T_init, iterations = 0, status = 0, every trace record {T_init, 0,
 *   0, 0, 0}, sums 0 and nn_idx -1 (one launch).  n == 0 (an empty grid) matches nothing: flag bit 1 at iteration 0.
 *   Launches: icp_accumulate then icp_solve per iteration, 2 * max_iter in all, on the given stream; no host synchronisation, no
 *   memset, no atomics: the call can be captured into a HIP graph as one linear chain.  icp_accumulate: one wave per source
 *   point, four per workgroup, at most 1024 workgroups striding over the points (the result does not depend on that number);
 *   every workgroup writes one row of 32 sums to the workspace; icp_solve adds the rows.  Integer sums: two runs are bitwise equal.
 *   Workspace: epn_icp_workspace_bytes(m) bytes (host-only; 0 outside 0 <= m <= 2^20), 16-byte aligned; written by the call and
 *   not read before it is written.  It must not be shared by two calls in flight.
 *   Refusals, decided before any HIP runtime call: EPN_EINVAL for n outside 0..2^22, m outside 0..2^20, max_dist not finite or
 *   <= 0, max_iter outside 0..1024, rel_fitness or rel_rmse negative or not finite, a grid_workspace address and n that no build
 *   was called with, or max_dist > max_radius of that build; then EPN_ENULL for T_init, T, iterations, status, src (m > 0) or
 *   trace (max_iter > 0) NULL; then EPN_EWORKSPACE for a workspace that is NULL, misaligned or too small. */
size_t epn_icp_workspace_bytes(int64_t m);
int epn_icp_refine_f32(const void *grid_workspace, int64_t n, const float *tgt_normals, const float *src, int64_t m,
                       const double *T_init, double max_dist, int max_iter, double rel_fitness, double rel_rmse, void *workspace,
                       size_t workspace_bytes, double *T, double *trace, int32_t *iterations, int32_t *status, int64_t *sums,
                       int32_t *nn_idx, epn_stream_t stream);

/* TSDF fusion: a window of depth frames -> the surface points of ONE fragment (csrc/tsdf_fusion.hip,
 * csrc/tsdf_math.h).  The reference makes its fragments on the host with open3d (SPConvNets/datasets/preprocess/run_fusion.py:20-49
 * with the settings of preprocess/tool.py:17-27): per window of frames_per_frag = 50 frames a ScalableTSDFVolume (voxel_length
 * 3.0 / 512, sdf_trunc 0.04, depth scale 1000, depth truncation 6 m) integrates every frame, then extract_point_cloud() and
 * estimate_normals() (which is epn_point_normals_f32).  This is open3d's algorithm made deterministic, positions only: no colour
 * (nothing downstream reads it) and not the extract's gradient normals (the reference overwrites them).  Differences from open3d a
 * maintainer should know: the arithmetic is fp64 from the fp32 depth on, where open3d's is float (and sdf / sdf_trunc is a
 * division where open3d multiplies by a reciprocal); the unit directory is a dense array over a caller-given box, not a hash map,
 * so a sample outside the box is flagged instead of allocated; blocks and points come in the fixed order below, where open3d's is
 * its hash map's; a sample touches the units of the CORNERS of its +- sdf_trunc box (the same set as open3d's box walk under the
 * sdf_trunc rule below).  Argued from open3d's algorithm, not run against it.
 * All arithmetic below is fp64 with every operation rounded on its own (no fma), written in the order to evaluate it, unless
 * it says fp32; a numpy restatement reproduces every output bit for bit (tests/tsdf_ref.py).
 *
 * epn_tsdf_fuse_f32: depth u16[F,H,W], cam2base f64[F,4,4] and base2cam f64[F,4,4] (row-major; each frame's pose in the first
 *   frame's coordinates and its inverse -- the caller inverts, the device never does; only the first three rows are read), the
 *   pinhole fx, fy, cx, cy, depth_scale, depth_trunc, voxel_length, sdf_trunc, stride (open3d's depth_sampling_stride: 4), the unit
 *   box lo_x.., dim_x.., max_blocks -> block_unit i32[max_blocks,3], block_mask u64[max_blocks], tsdf f32[max_blocks,16,16,16],
 *   weight i32[max_blocks,16,16,16] (outputs, not scratch: they are what makes the entry testable; both 16-byte aligned), status
 *   i32[4] = {n_blocks, flags, n_outside, 0}, all on the device.
 *   depth           d = (float)raw / (float)depth_scale, one fp32 division; d = 0 where raw == 0 or (double)d > depth_trunc.  0 means
 *                   "no measurement".  Everything after is fp64 from this fp32 value.
 *   units           a unit is 16^3 voxels (open3d's volume_unit_resolution), unit_length = 16 * voxel_length; the unit index of a
 *                   coordinate is floor(x / unit_length): floor, not truncation.  The directory is a dense array of 64-bit frame
 *                   masks over the box of units lo <= unit < lo + dim per axis, entry ((ux - lo_x) dim_y + (uy - lo_y)) dim_z +
 *                   (uz - lo_z); a non-zero mask means "allocated".  There is no hash table: ranks come from a prefix sum
 *                   over the directory in this linear order, so nothing depends on arrival order.
 *   touch           (ScalableTSDFVolume::Integrate, first half) every pixel (u, v) with u % stride == 0, v % stride == 0 and d != 0:
 *                   c = (((u - cx) * d) / fx, ((v - cy) * d) / fy, d); p_i = ((T_i0 c_0 + T_i1 c_1) + T_i2 c_2) + T_i3 with T =
 *                   cam2base[f]; per axis lo_i = floor((p_i - sdf_trunc) / unit_length), hi_i = floor((p_i + sdf_trunc) /
 *                   unit_length); bit f is set (64-bit atomicOr: order-independent) in every unit of {lo_0, hi_0} x {lo_1, hi_1} x
 *                   {lo_2, hi_2}.  sdf_trunc <= 8 * voxel_length is required, so that these corners are the whole index box (at
 *                   most 2 units per axis).  A unit outside the caller's box (or a non-finite index) is not allocated: flags bit
 *                   0 is raised and n_outside counts the samples (pixel, frame) with at least one such unit.  Nothing is
 *                   dropped silently.
 *   blocks          the allocated units take ranks 0..n_blocks-1 in ascending directory order; block_unit[r] = the unit's index,
 *                   block_mask[r] = its mask.  n_blocks > max_blocks raises flags bit 1; ranks >= max_blocks are neither
 *                   integrated nor written (rows past min(n_blocks, max_blocks) are left untouched), and the extract treats them
 *                   as absent.
 *   integrate       (UniformTSDFVolume::IntegrateWithDepthToCameraDistanceMultiplier) per voxel (x, y, z) of a block, (tsdf, w) =
 *                   (0, 0), then for exactly the frames of the block's mask in ascending f (open3d integrates only the units the
 *                   current frame touched):
 *                   1. centre_i = ((16 unit_i + idx_i) + 0.5) * voxel_length;
 *                   2. c = the centre under base2cam[f], summed as in touch;
 *                   3. skip unless c_2 > 0;
 *                   4. u_f = ((c_0 * fx) / c_2 + cx) + 0.5, v_f = ((c_1 * fy) / c_2 + cy) + 0.5; skip unless 0 <= u_f < W and
 *                      0 <= v_f < H; pixel (pu, pv) = ((int)u_f, (int)v_f);
 *                   5. skip when that pixel's d == 0;
 *                   6. a = (pu - cx) / fx, b = (pv - cy) / fy, sdf = (d - c_2) * sqrt((a a + b b) + 1); skip unless sdf >
 *                      -sdf_trunc (strict);
 *                   7. t = (float)min(1, sdf / sdf_trunc); then in fp32, each operation rounded on its own, tsdf = (tsdf * (float)w
 *                      + t) / (float)(w + 1); w += 1.
 *                   A voxel no frame observed keeps (0, 0).  tsdf and weight are indexed [block][x][y][z], z fastest.
 * epn_tsdf_extract_f32: tsdf, weight, block_unit, the box and max_blocks of a fuse and its workspace (which holds n_blocks and the
 *   directory's ranks) -> points f32[max_points,3], status i32[2] = {M, flags}.  (ScalableTSDFVolume::ExtractPointCloud, positions.)
 *   A voxel takes part when w != 0 and -0.98f <= tsdf < 0.98f (fp32 comparisons).  For a voxel that takes part, with value f0 and
 *   centre p, and each axis a = 0, 1, 2: its +1 neighbour on that axis -- looked up through the directory when it lies in the
 *   next unit; an absent unit, a unit outside the box or a rank >= min(n_blocks, max_blocks) gives no neighbour -- must take part
 *   too, with value f1; a point is emitted where (double)f0 * (double)f1 < 0, with coordinate (p_a r1 + (p_a + voxel_length) r0) /
 *   (r0 + r1) on axis a, r0 = |f0|, r1 = |f1|, and p on the other two; stored as fp32.  Order: ascending block rank, then voxel
 *   x, y, z with z fastest, then axis 0, 1, 2 (per-block counts, one scan, the write pass).  M > max_points raises flags bit 0
 *   and nothing is written beyond max_points rows.
 * Workspace: epn_tsdf_fuse_workspace_bytes(F, H, W, stride, dim_x, dim_y, dim_z, max_blocks) bytes (host-only; 0 for arguments the
 *   fuse refuses: 64 + 12 bytes per directory entry + 4 per block, tile and touch workgroup), 8-byte aligned, initialised by the
 *   fuse itself and read by the extract.  Launches: fuse six (init, touch, count, scan, rank, integrate -- one workgroup per
 *   block, frames looped inside), extract three.  The only atomic is the touch's 64-bit OR; no floating-point atomics; no loop
 *   bound depends on data; every directory, pool and pixel index is range-checked where it is read; two runs are bitwise equal.
 * Refusals, decided before any HIP runtime call: EPN_EINVAL for F outside 1..64, H or W outside 1..16384, stride < 1, a
 *   non-finite or non-positive fx, fy, depth_scale (also as a float), depth_trunc, voxel_length or sdf_trunc, a non-finite cx or
 *   cy, sdf_trunc > 8 * voxel_length, a dimension < 1, a box product over 2^24, |lo| > 2^24, max_blocks outside 1..2^17 (2^17
 *   blocks hold fewer than 2^31 points), max_points < 0, tsdf or weight not 16-byte aligned; then EPN_ENULL for a NULL pointer
 *   (points only when max_points > 0); then EPN_EWORKSPACE for a workspace that is NULL, not 8-byte aligned or too small. */
size_t epn_tsdf_fuse_workspace_bytes(int F, int H, int W, int stride, int dim_x, int dim_y, int dim_z, int max_blocks);
int epn_tsdf_fuse_f32(const uint16_t *depth, int F, int H, int W, const double *cam2base, const double *base2cam, double fx,
                      double fy, double cx, double cy, double depth_scale, double depth_trunc, double voxel_length,
                      double sdf_trunc, int stride, int lo_x, int lo_y, int lo_z, int dim_x, int dim_y, int dim_z, int max_blocks,
                      int32_t *block_unit, uint64_t *block_mask, float *tsdf, int32_t *weight, int32_t *status, void *workspace,
                      size_t workspace_bytes, epn_stream_t stream);
int epn_tsdf_extract_f32(const float *tsdf, const int32_t *weight, const int32_t *block_unit, int max_blocks, int lo_x, int lo_y,
                         int lo_z, int dim_x, int dim_y, int dim_z, double voxel_length, float *points, int max_points,
                         int32_t *status, void *workspace, size_t workspace_bytes, epn_stream_t stream);

/* Rotation estimation: what turns RegSO3ConvModel's head output into a rotation, the labels a training step needs and the
 * angular error the reference reports.  All tensors are contiguous device memory, float or int32; anchors
 * f32[A,3,3], 1 <= A <= 64.  Arithmetic is fp64 on the fp32 inputs and every output is rounded once to fp32.  One wave per
 * pair, lane a owns source anchor a; sums over lanes are a fixed xor tree, so results are bitwise repeatable.  No workspace, no
 * atomics, every loop bounded by A, N or a fixed sweep count.  A pair with non-finite inputs leaves its own rows unspecified
 * (its preds still lie in 0..A-1) and touches nothing else.
 * Refusals, decided before any HIP runtime call: EPN_EINVAL for b < 0, A outside 1..64, nr not 4 or 6, N < 1; then b == 0
 * succeeds and launches nothing; then EPN_ENULL for a required pointer that is NULL.
 *
 * epn_rotation_labels_f32 (label_relative_rotation_np, vgtk/vgtk/functional/rotation.py:521-526, per pair on the device in
 *   place of Dataloader_ModelNet40Alignment's per-sample numpy, SPConvNets/datasets/modelnet40.py:152): T f32[b,3,3] ->
 *   R_target f32[b,A,3,3], label i32[b,A].  M(a,i) = A_a^T T A_i; label[a] = the i with the largest tr M(a,i), the lowest
 *   such i on a tie (compared in fp64); R_target[a] = M(a, label[a]).
 *
 * epn_so3_mean_f32 (so3_mean, rotation.py:481-518, without torch.svd): Rs f32[b,N,3,3], weights f32[b,N] or NULL (all ones)
 *   -> R f32[b,3,3], margin f32[b].  Ce = sum_n w_n Rs_n (lane l adds n = l, l + 64, ... in ascending order, then the tree).
 *   R is the rotation that maximises tr(R^T Ce): U diag(1, 1, det(U V^T)) V^T of Ce's singular value decomposition,
 *   Ce = U diag(s1 >= s2 >= s3) V^T.  margin = (s2 + det(U V^T) s3) / s1, the conditioning of that projection: R moves by at
 *   most 2 |dCe| / (s1 margin) under a perturbation dCe, and is not unique at margin 0.  Ce exactly zero: R = I, margin = 0.
 *   Method: tr(R(q)^T Ce) = q^T K q for the unit quaternion q of R, K the symmetric 4 x 4 matrix of Horn's closed form; its
 *   eigenvalues are s1 + s2 + d s3 >= s1 - s2 - d s3 >= ..., so q is the top eigenvector (cyclic Jacobi, 12 sweeps),
 *   s1 = (l1 + l2) / 2 and margin = (l1 - l2) / (l1 + l2).  R is always a rotation, whatever the margin.
 *
 * epn_rotation_decode_f32 (the alignment branch of MultiTaskDetectionLoss.forward without the loss, vgtk/vgtk/loss.py:140-172
 *   and :210-218, with batched_select_anchor :77-92 and the two rotation maps rotation.py:379-417, :443-478):
 *   wts f32[b,A,A] (target anchor, source anchor), y f32[b,nr,A,A], label i32[b,A] or NULL, gt_T f32[b,3,3] or NULL ->
 *   pred_R f32[b,3,3], preds i32[b,A], conf f32[b,A], margin f32[b], pred_Rs f32[b,A,3,3] (or NULL: not wanted),
 *   hits i32[b] (required and written iff label is given), err f32[b] (required and written iff gt_T is given).
 *     preds[a]  = arg max over t of wts[t,a], fp32 comparison: t = 0 first, replaced on a strict >, so the lowest t wins a tie
 *     c[a]      = wts[preds[a], a];  conf[a] = c[a] / (1e-6 + sum_a c[a])
 *     R_a       = rotation map of y[:, preds[a], a].  nr = 4: q = (w,x,y,z) / max(|q|, 1e-8), rows
 *                 (1-2yy-2zz, 2xy-2zw, 2xz+2yw), (2xy+2zw, 1-2xx-2zz, 2yz-2xw), (2xz-2yw, 2yz+2xw, 1-2xx-2yy).  nr = 6:
 *                 x = n(y[0:3]), z = n(x cross y[3:6]), y' = z cross x, columns (x, y', z), n(v) = v / max(|v|, 1e-8).
 *     pred_Rs[a] = A_a R_a A_preds[a]^T  (the einsum 'baij,bajk,balk->bail')
 *     pred_R, margin = the projection above of sum_a conf[a] pred_Rs[a] (unrounded conf and pred_Rs)
 *     hits      = the number of a with preds[a] == label[a]
 *     err       = acos_safe(0.5 (sum_ij pred_R_ij gt_T_ij - 1)) on the unrounded pred_R, acos_safe(x) = acos(x) for
 *                 |x| <= 1 - 1e-4 and acos(s (1 - 1e-4)) - s (|x| - 1 + 1e-4) acos(1 - 1e-4) / 1e-4, s = sign(x), beyond
 *                 (vgtk/vgtk/spconv/functional.py:138-143). */
int epn_rotation_labels_f32(const float *anchors, const float *T, int b, int A, float *R_target, int32_t *label,
                            epn_stream_t stream);
int epn_so3_mean_f32(const float *Rs, const float *weights, int b, int N, float *R, float *margin, epn_stream_t stream);
int epn_rotation_decode_f32(const float *wts, const float *y, const float *anchors, const int32_t *label, const float *gt_T,
                            int b, int A, int nr, float *pred_R, int32_t *preds, float *conf, float *margin, float *pred_Rs,
                            int32_t *hits, float *err, epn_stream_t stream);

/* The rotation network's training loss: the alignment branch of MultiTaskDetectionLoss.forward (vgtk/vgtk/loss.py:140-181,
 * with CrossEntropyLoss :18-30 and batched_select_anchor :77-92) and its backward (csrc/rotation_loss.hip).
 * All tensors are contiguous device memory, float or int32: wts f32[b,A,A] (target anchor t, source anchor a), y f32[b,nr,A,A],
 * label i32[b,A], R_target f32[b,A,3,3] (the reference's gt_R: epn_rotation_labels_f32's R_target), 1 <= A <= 64, nr = 4 or 6,
 * w the weight of the L2 term.  Arithmetic is fp64 on the fp32 inputs and every output is rounded once to fp32.  No workspace, no
 * atomics, no host synchronisation (the calls can be captured into a HIP graph); every sum runs in a fixed order, so two runs
 * are bitwise equal.
 * Refusals, decided before any HIP runtime call: EPN_EINVAL for b < 0, A outside 1..64, nr not 4 or 6, a non-finite w; then
 * b == 0 succeeds and launches nothing; then EPN_ENULL for a pointer that is NULL (all are required).
 *
 * epn_rotation_loss_f32: for every pair p and source anchor a (a "row"), with L = label[p,a]:
 *     row_flags bit 0: L lies outside 0..A-1.  Such a row is never used as an address: its row_ce and row_l2 are 0, its sel_R
 *               is zero, bit 1 is clear and it contributes zero gradient.  It stays in the divisors below.
 *     preds     = arg max over t of wts[p,t,a], fp32 comparison, the lowest t on a tie: epn_rotation_decode_f32's rule, so
 *               the two entries agree on every input
 *     row_ce    = m + log(sum_t exp(wts[p,t,a] - m)) - wts[p,L,a], m the maximum over t, t ascending: torch.nn.CrossEntropyLoss
 *               on wts as logits with the class axis at dim 1, as the reference applies it
 *     sel_R     = the rotation map of y[p,:,L,a], exactly as specified for epn_rotation_decode_f32 (one device function serves
 *               both): nr = 4 the quaternion formula, nr = 6 the Gram-Schmidt form, n(v) = v / max(|v|, 1e-8)
 *     row_flags bit 1: a norm entering that map (nr = 4: |q|; nr = 6: |y[0:3]| or |x cross y[3:6]|) was below 1e-8
 *     row_l2    = sum_ij (R_target[p,a,i,j] - sel_R[p,a,i,j])^2 on the unrounded sel_R, added in row-major order
 *   -> row_ce, row_l2 f32[b,A], preds, row_flags i32[b,A], sel_R f32[b,A,3,3] and scalars f32[4] = (loss, cls_loss, reg, r_acc),
 *   the first four values of the reference's return tuple:
 *     cls_loss = sum row_ce / (b A);  reg = w sum row_l2 / (9 b A);  loss = cls_loss + reg;  r_acc = #{preds == label} / (b A)
 *   The sums run in fp64 over the ROUNDED per-row outputs (thread i of one workgroup adds rows i, i + 256, ... ascending, then
 *   a fixed tree); cls_loss, reg and their fp64 sum are each rounded once.  Two launches; one wave per pair, lane a owns
 *   source anchor a.
 *
 * epn_rotation_loss_bwd_f32: upstream f32[1] (the gradient of scalars[0], on the device), the forward's inputs and its row_flags
 *   -> dwts f32[b,A,A], dy f32[b,nr,A,A], EVERY element written (zeros explicitly: the caller needs no memset).  With g = upstream:
 *     dwts[p,t,a]  = g / (b A) (softmax_t(wts[p,.,a]) - [t == L]);  0 for every t of a row with bit 0 set
 *     dy[p,:,t,a]  = 0 for t != L;  dy[p,:,L,a] = J^T vec(G), G = g 2 w / (9 b A) (sel_R - R_target), J the Jacobian of the
 *                    rotation map at y[p,:,L,a]: through v / |v| where the norm was >= 1e-8, (I - u u^T) / |v| with u = v / |v|;
 *                    through v / 1e-8 where the clamp was active (what autograd makes of torch.max(norm, 1e-8))
 *   The softmax and sel_R are recomputed from the inputs in fp64 (the fp32 sel_R is not read).  The label is range-checked on
 *   the device again before it is used as an address.  One launch. */
int epn_rotation_loss_f32(const float *wts, const float *y, const int32_t *label, const float *R_target, int b, int A, int nr,
                          double w, float *row_ce, float *row_l2, int32_t *preds, int32_t *row_flags, float *sel_R,
                          float *scalars, epn_stream_t stream);
int epn_rotation_loss_bwd_f32(const float *upstream, const float *wts, const float *y, const int32_t *label,
                              const float *R_target, const int32_t *row_flags, int b, int A, int nr, double w, float *dwts,
                              float *dy, epn_stream_t stream);

/* The classification network's training loss and evaluation tallies: CrossEntropyLoss and AttentionCrossEntropyLoss
 * (vgtk/vgtk/loss.py:18-75) and the counting of the evaluation loop (SPConvNets/trainer_modelnet.py:138-210, its commented-out
 * class x anchor table included); csrc/cls_loss.hip.  The class term and the attention term are the same
 * problem: rows of n contiguous fp32 logits with one int32 label per row.  Class set: logits f32[B,k], label i32[B].  Attention
 * set: att f32[R,A], att_label i32[R]; absent as a whole with R == 0 (plain CrossEntropyLoss: its pointers and A are not looked
 * at).  For the reference's two layouts of wts: [B,A] is R = B rows; [B,C,A] is R = B C rows, row b C + c labelled rlabel[b,c].
 * coef f32[2] = (c_cls, c_att) is DEVICE memory, read by the kernels in both directions: a captured step replays with new blend
 * weights after an in-place update of those two floats.  All tensors are contiguous device memory.  Arithmetic is fp64 on the
 * fp32 inputs and every output is rounded once.  No workspace, no float atomics, no host synchronisation; every float sum runs
 * in a fixed order, so two runs are bitwise equal.
 * Refusals, decided before any HIP runtime call: EPN_EINVAL for B outside 1..65536, k outside 1..4096, R outside 0..65536, A
 * outside 1..4096 when R > 0, B k or R A >= 2^31 (tally: A is checked when att_pred is given); then EPN_ENULL for a required
 * pointer that is NULL.
 *
 * epn_cls_loss_f32: per row x[0..n) of either set, with L its label:
 *     row_flags bit 0: L lies outside 0..n-1 (torch asserts on the device there).  The row's row_ce is 0 and its gradient is
 *               zero; it STAYS in the divisors B and R -- unlike torch's ignore_index = -100, which shrinks the divisor.
 *     row_flags bit 1: an element of the row is not finite (NaN, +inf or -inf).  pred = -1; row_ce = NaN and the gradient is NaN
 *               unless bit 0 is set as well, which wins for both.
 *     pred      = arg max_j x[j], fp32 comparison, the LOWEST j on a tie
 *     row_ce    = lse - x[L] with lse = m + log(sum_j exp(x[j] - m)), m the maximum; evaluated as (m - x[L]) + log(sum), whose
 *               first term is exact, j ascending per lane (lane l adds j = l, l + 64, ...), then a fixed xor tree over the lanes
 *   -> row_ce f32, pred i32, flags i32 per row of each set, and scalars f32[5] = (loss, cls_loss, att_loss, acc, att_acc):
 *     cls_loss = sum row_ce / B;  att_loss = sum att_row_ce / R;  acc = #{pred == label and pred >= 0} / B, att_acc alike over R;
 *     loss = c_cls cls_loss + c_att att_loss.  With R == 0: att_loss = att_acc = 0 and loss = c_cls cls_loss.
 *   The sums run in fp64 over the ROUNDED per-row outputs (thread i of one workgroup adds rows i, i + 256, ... ascending, then a
 *   fixed tree); each scalar is rounded once.  Two launches; one wave per row.
 *
 * epn_cls_loss_bwd_f32: upstream f32[1] (the gradient of scalars[0], on the device), the forward's inputs and its two flag arrays
 *   -> dlogits f32[B,k], datt f32[R,A], EVERY element written.  With g = upstream:
 *     dlogits[b,j] = g c_cls / B (softmax_j(logits[b,.]) - [j == label[b]]);  datt[r,j] = g c_att / R (softmax_j(att[r,.]) - [j == L_r])
 *   the factor formed first, in that order, in fp64; the softmax recomputed in fp64 as above.  Rows with bit 0: zeros.  Other
 *   rows with bit 1: NaN.  c_att == 0 writes datt as (signed) zeros; it is not skipped.  The label is range-checked again on the
 *   device.  One launch.
 *
 * epn_cls_tally_i32: pred, label, flags i32[B] of the class set; optionally att_pred, att_flags i32[B] (the [B,A] layout only:
 *   one attention row per cloud) and with them optionally att_label i32[B]; ADDS into caller-owned, caller-zeroed tables
 *     confusion i32[k,k] at (label, pred);  anchor_table i32[k,A] at (label, att_pred) -- upstream's lmc, required with att_pred;
 *     totals i32[4] = rows seen, rows with pred == label, rows with att_pred == att_label, rows skipped.
 *   A row with any flag bit set in either flag array is skipped and counted in totals[3]; so is a row whose label or pred lies
 *   outside 0..k-1 or whose att_pred lies outside 0..A-1 (nothing read from memory becomes an address unchecked).  Integer
 *   atomics: integer addition does not depend on the order, so the tables are bitwise repeatable.  One launch. */
int epn_cls_loss_f32(const float *logits, const int32_t *label, int B, int k, const float *att, const int32_t *att_label, int R,
                     int A, const float *coef, float *row_ce, int32_t *pred, int32_t *flags, float *att_row_ce, int32_t *att_pred,
                     int32_t *att_flags, float *scalars, epn_stream_t stream);
int epn_cls_loss_bwd_f32(const float *upstream, const float *logits, const int32_t *label, const int32_t *flags, int B, int k,
                         const float *att, const int32_t *att_label, const int32_t *att_flags, int R, int A, const float *coef,
                         float *dlogits, float *datt, epn_stream_t stream);
int epn_cls_tally_i32(const int32_t *pred, const int32_t *label, const int32_t *flags, const int32_t *att_pred,
                      const int32_t *att_label, const int32_t *att_flags, int B, int k, int A, int32_t *confusion,
                      int32_t *anchor_table, int32_t *totals, epn_stream_t stream);

/* Adam over every parameter of a model in one call: the optimiser of the three trainers (optim.Adam driven by
 * vgtk.LearningRateScheduler, vgtk/vgtk/app/trainer.py:162-168); csrc/adam_step.hip.  Two launches, no host
 * synchronisation, no allocation, no float atomics; capturable on one stream; two runs from equal state are bitwise equal.
 * amsgrad is not built.
 * Operands, all contiguous fp32 device memory: nseg parameter segments, reached through seg_param u64[nseg] (their device
 * addresses, each 4-byte aligned; the parameters stay where they are) and seg_off i64[nseg + 1] (seg_off[0] = 0, strictly
 * increasing, seg_off[nseg] = n: segment s is the flat range seg_off[s] .. seg_off[s + 1] - 1), both tables in DEVICE memory;
 * three flat buffers of n elements that share those offsets: grad (read only), exp_avg, exp_avg_sq.  A segment may start at any
 * 4-byte boundary; 16-byte accesses are used where the flat buffers and the parameter's address allow them, per four elements.
 * lr f32[1] is DEVICE memory, read by the kernel: a captured step replays with a new rate after an in-place write of that float.
 * counters i32[2] = (steps_applied, steps_skipped), caller-zeroed at the start of training; info f32[4] is written by every call.
 *
 * The flat index space is cut into chunks of EPN_ADAM_SPAN elements, contiguous runs of chunks per workgroup, the partition
 * fixed by n alone.  With s = grad_scale:
 *   pass A  sumsq = sum (s g)^2 in fp64 (per thread ascending, a fixed tree per workgroup, one partial per workgroup into the
 *           workspace) and the number of non-finite elements of g; steps_applied is copied into the workspace.
 *   pass B  every workgroup adds the partials in one fixed order (the same bits in all of them) and forms
 *             norm = sqrt(sumsq);  skip = (nonfinite > 0) or not finite(norm);
 *             c = 1 when max_norm <= 0 or max_norm = +inf, else max_norm / (norm + 1e-6) where that is < 1, else 1 (a NaN
 *             quotient gives 1): the rule of torch's clip_grad_norm_.
 *           info = (norm, c, lr as read, skip as 0 or 1), each rounded once.  With skip set, steps_skipped grows by one and
 *           NOTHING else is written: p, exp_avg, exp_avg_sq and steps_applied keep their bits.  Otherwise steps_applied becomes
 *           t = steps_applied + 1 (written by one workgroup; all read the copy pass A made, so none sees the new value), and per
 *           element, in fp64 on the fp32 inputs, no fused multiply-add, every stored value rounded once to nearest with
 *           subnormals kept:
 *             g' = (s c) g + weight_decay p
 *             m' = fl32(beta1 m + (1 - beta1) g')
 *             v' = fl32(beta2 v + (1 - beta2) (g' g'))
 *             p' = fl32(p - ((lr / (1 - beta1^t)) m') / (sqrt(v') / sqrt(1 - beta2^t) + eps))
 *           p' is formed from the ROUNDED m' and v': the stored state determines the next step, as in torch.optim.Adam.
 * A finite gradient cannot overflow sumsq: n < 2^40 squares below 2^256 stay below 2^296.
 *
 * epn_adam_workspace_bytes(n): host only; positive, never decreasing in n.  The workspace needs 8-byte alignment.
 * epn_adam_check_plan: host only, on HOST copies of the two tables.  EPN_EINVAL unless 1 <= nseg <= 65536, seg_off[0] == 0, the
 *   offsets increase strictly, seg_off[nseg] == n, 1 <= n < 2^40 and every address is non-zero and 4-byte aligned (EPN_ENULL
 *   for a NULL table).
 * epn_adam_step_f32 refusals, decided before any HIP runtime call: EPN_EINVAL for nseg outside 1..65536, n outside 1..2^40 - 1,
 *   nseg > n, beta1 or beta2 outside [0, 1), eps <= 0, a negative or non-finite eps, weight_decay or grad_scale (NaN included),
 *   a NaN max_norm; then EPN_ENULL for seg_param, seg_off, grad, exp_avg, exp_avg_sq, lr, counters or info NULL; then
 *   EPN_EWORKSPACE for a workspace that is NULL, misaligned or smaller than epn_adam_workspace_bytes(n).  The device tables are
 *   not read on the host: validate them with epn_adam_check_plan when they are built. */
#define EPN_ADAM_SPAN 1024
size_t epn_adam_workspace_bytes(long long n);
int epn_adam_check_plan(const unsigned long long *seg_param, const long long *seg_off, int nseg, long long n);
int epn_adam_step_f32(const unsigned long long *seg_param, const long long *seg_off, int nseg, long long n, const float *grad,
                      float *exp_avg, float *exp_avg_sq, const float *lr, double beta1, double beta2, double eps,
                      double weight_decay, double grad_scale, double max_norm, int32_t *counters, float *info, void *workspace,
                      size_t workspace_bytes, epn_stream_t stream);

/* The descriptor network's training loss: batch-hard triplet mining and the anchor interpolation of its equivariance term
 * (csrc/triplet_loss.hip).  All tensors are contiguous device memory, float or int32.  Arithmetic is fp64 on
 * the fp32 inputs and every output is rounded once to fp32.  No workspace, no atomics, no host synchronisation (the calls can
 * be captured into a HIP graph); every sum runs in a fixed order, so two runs are bitwise equal.  The N x N distance matrix is
 * never written.
 * Refusals, decided before any HIP runtime call: EPN_EINVAL for N outside 2..65536 (the reference's mining fails on N = 1 too:
 * there is no negative), D < 1, N * D >= 2^31, an unknown mode, eps <= 0, a non-finite margin (soft: margin <= 0), C < 1,
 * A not 12 or 60, knn != 3, nb < 0, nb * C * A >= 2^31, sigma <= 0; nb == 0 succeeds and launches nothing; then EPN_ENULL for
 * a pointer that is NULL (all are required).
 *
 * epn_triplet_batch_hard_f32 (pairwise_distance_matrix, batch_hard_negative_mining and
 *   TripletBatchLoss._forward_invariance, vgtk/vgtk/loss.py:220-235 and :280-318): src, tgt f32[N,D]; mode one of
 *   EPN_TRIPLET_*; margin; eps (the reference's 1e-6).
 *     d2(i,j)   = sum_d (src[i,d] - tgt[j,d])^2: the difference formed in fp64, the terms added in ascending d with one fused
 *                 multiply-add each.  Equal in exact arithmetic to the reference's |x|^2 + |y|^2 - 2 x.y, without the
 *                 cancellation that form suffers where unit descriptors are close.
 *     dist(i,j) = sqrt(d2 < eps ? eps : d2)
 *     d_pos[i]  = dist(i,i);  d_neg[i] = min over j != i of dist(i,j), neg_idx[i] the lowest such j;
 *     nn_idx[i] = the lowest j with the smallest dist(i,j) over all j
 *     row_loss  hard: max(d_pos - d_neg + margin, 0);  soft: x = d_pos - d_neg, x if margin x > 20, else
 *               log1p(exp(margin x)) / margin (torch's softplus with beta = margin);  contrastive: d_pos + max(margin - d_neg, 0)
 *     row_flags bit 0: d2(i,i) < eps; bit 1: d2(i,neg_idx[i]) < eps; bit 2: the hinge is active (hard: d_pos - d_neg + margin
 *               > 0; contrastive: margin - d_neg > 0; soft: always set) -- decided on the unrounded values
 *   -> d_pos, d_neg, row_loss f32[N], neg_idx, nn_idx, row_flags i32[N] (outputs, not scratch: the backward reads them and they
 *   are what makes the entry testable) and scalars f32[4] = mean row_loss, #{i: nn_idx[i] == i} / N, mean d_pos, mean d_neg,
 *   each the fp64 mean of the ROUNDED per-row outputs (thread t adds rows t, t + 256, ... ascending, then a fixed tree),
 *   rounded once.  Two launches.  neg_idx and nn_idx lie in 0..N-1 and neg_idx[i] != i for any input, NaN included.
 *
 * epn_triplet_batch_hard_bwd_f32: upstream f32[1] (the gradient of scalars[0], on the device), src, tgt and the per-row outputs
 *   above -> dsrc, dtgt f32[N,D], every element written.  With x = d_pos - d_neg,
 *     hard: gp = gn = bit 2;  soft: gp = gn = 1 if margin x > 20, else 1 / (1 + exp(-margin x));  contrastive: gp = 1, gn = bit 2
 *     cp[i] = bit 0 ? 0 : upstream gp / (N d_pos[i]);  cn[i] = bit 1 ? 0 : upstream gn / (N d_neg[i])
 *     dsrc[i] = cp[i] (src[i] - tgt[i]) - cn[i] (src[i] - tgt[neg_idx[i]])
 *     dtgt[j] = -cp[j] (src[j] - tgt[j]) + sum over the i with neg_idx[i] == j, in ascending i, of cn[i] (src[i] - tgt[j])
 *   (a clamped distance and an inactive hinge give zero, as torch.clamp and relu do).  dtgt is a gather: the workgroup of row
 *   j scans neg_idx[0..N).  A neg_idx entry outside 0..N-1 is never used as an address (its row contributes no negative
 *   term).  One launch.
 *
 * epn_anchor_interp_f32 (TripletBatchLoss._interpolate and _rotation_distance, loss.py:400-445, gathering per sample as the
 *   commented-out line :427 intends; the reference's own line :424 fails for nb >= 2): feature f32[nb,C,A], T f32[nb,3,3],
 *   anchors f32[A,3,3], A = 12 or 60, knn = 3, sigma > 0.  Per sample b and anchor n:
 *     trace[m]  = tr(T_b^T A_n A_m^T), P = T_b^T A_n in fp64, then the nine products added in row-major order
 *     idx[n,0..2] = the three m with the largest trace in descending order, the lower m first on a tie
 *     w[n,k]    = exp((trace_k - trace_0) / sigma) / sum_k exp((trace_k - trace_0) / sigma)
 *     out[b,c,n] = sum_k w[n,k] feature[b,c,idx[n,k]] (k ascending, unrounded w)
 *   -> out f32[nb,C,A], idx i32[nb,A,3], w f32[nb,A,3].  idx lies in 0..A-1 for any input.  One launch, one workgroup per sample.
 *
 * epn_anchor_interp_bwd_f32: dout f32[nb,C,A], idx, w as written above -> dfeature f32[nb,C,A], every element written:
 *     dfeature[b,c,m] = sum over the entries (n,k) with idx[n,k] == m, in ascending 3 n + k, of w[n,k] dout[b,c,n]
 *   a gather over the 3 A saved entries (idx is only compared, never an address).  T gets no gradient.  One launch. */
#define EPN_TRIPLET_HARD 0
#define EPN_TRIPLET_SOFT 1
#define EPN_TRIPLET_CONTRASTIVE 2
int epn_triplet_batch_hard_f32(const float *src, const float *tgt, int N, int D, int mode, double margin, double eps,
                               float *d_pos, float *d_neg, float *row_loss, int32_t *neg_idx, int32_t *nn_idx,
                               int32_t *row_flags, float *scalars, epn_stream_t stream);
int epn_triplet_batch_hard_bwd_f32(const float *upstream, const float *src, const float *tgt, const float *d_pos,
                                   const float *d_neg, const int32_t *neg_idx, const int32_t *row_flags, int N, int D, int mode,
                                   double margin, float *dsrc, float *dtgt, epn_stream_t stream);
int epn_anchor_interp_f32(const float *feature, const float *T, const float *anchors, int nb, int C, int A, int knn, double sigma,
                          float *out, int32_t *idx, float *w, epn_stream_t stream);
int epn_anchor_interp_bwd_f32(const float *dout, const int32_t *idx, const float *w, int nb, int C, int A, int knn,
                              float *dfeature, epn_stream_t stream);

/* ------------------------------------------------------------------ InterSO3Conv ------------ */

/* Geometry + shapes of one inter convolution (vgtk/vgtk/so3conv/functional.py:118-178).
 * The fused kernels regenerate the kernel-influence weights
 *     w[b,p,a,k,n] = relu(1 - |xyz[:,idx[b,p,n]] - new_xyz[:,p] - R_a kappa_k|^2 / sigma)
 * (functional.py:180-218) on the fly; they are never written to HBM. */
typedef struct epn_inter_desc {
    const float *xyz;        /* [b,3,p1] support coordinates                                   */
    const float *new_xyz;    /* [b,3,p2] query (output) coordinates                            */
    const int32_t *ball_idx; /* [b,p2,nn] neighbour indices into p1 (from epn_ball_query_f32)  */
    const float *anchors;    /* [na,3,3] rotation matrices                                     */
    const float *kernels;    /* [ks,3]   kernel points                                         */
    const float *dense_w;    /* optional [b,p2,na,ks,nn]: use THESE weights instead of geometry */
    float sigma;
    int b, p1, p2, nn, na, ks, cin, cout;
} epn_inter_desc;

/* Bytes of scratch the inter kernels need for this descriptor (tables; plus the materialised
 * grouped features on the generic path used when cin or cout is not a multiple of 16). */
size_t epn_inter_workspace_bytes(const epn_inter_desc *d);

/* Replaces InterSO3Conv.forward's compute (vgtk/vgtk/so3conv/modules.py:157-174 =
 * inter_so3conv_grouping -> inter_zpconv_grouping_naive (vgtk/vgtk/spconv/functional.py:372-390)
 * -> BasicSO3Conv (modules.py:48-55)):
 *   out_cl[b,p,a,o] = sum_{c,k} W[o, c*ks+k] * sum_n feats_cl[b, idx[b,p,n], a, c] * w[b,p,a,k,n]
 * feats_cl f32[b,p1,na,cin], W f32[cout, cin*ks] -> out_cl f32[b,p2,na,cout]. */
int epn_inter_so3conv_fwd_f32(const epn_inter_desc *d, const float *feats_cl, const float *W,
                              float *out_cl, void *workspace, size_t workspace_bytes,
                              epn_stream_t stream);

/* Autograd transposes (reference: torch autograd through gather/einsum/matmul).
 * grad_out_cl f32[b,p2,na,cout].
 *   bwd_data  : grad_feats_cl f32[b,p1,na,cin]  (zero-filled here, then accumulated)
 *   bwd_weight: grad_W f32[cout, cin*ks]        (zero-filled here, then accumulated) */
int epn_inter_so3conv_bwd_data_f32(const epn_inter_desc *d, const float *grad_out_cl,
                                   const float *W, float *grad_feats_cl, void *workspace,
                                   size_t workspace_bytes, epn_stream_t stream);
int epn_inter_so3conv_bwd_weight_f32(const epn_inter_desc *d, const float *feats_cl,
                                     const float *grad_out_cl, float *grad_W, void *workspace,
                                     size_t workspace_bytes, epn_stream_t stream);

/* The first layer of every model (cin = 1: the occupancy feature of get_occupancy_features, so3conv/functional.py:25-44;
 * InterSO3Conv(1 -> cout), cls_so3net_pn.py:101) is not matrix work: its cost is generating the ks x nn kernel-influence
 * weights per column on the VALU -- and round 3's weight gradient paid it a second time.  These two entry points keep the
 * 24 grouped values of a column (`grouped` f32[b*p2*na][ks], 96 bytes per column: 94 MB at B=32 against the 3 GB inter_w
 * the reference keeps for the same purpose) from the forward pass, and the weight gradient contracts grad_out with them:
 *   epn_inter_so3conv_fwd_c1_f32        : as epn_inter_so3conv_fwd_f32 for cin = 1; `grouped` may be NULL (inference)
 *   epn_inter_so3conv_bwd_weight_c1_f32 : grad_W f32[cout][ks] = grad_out^T . grouped (zero-filled here, then accumulated)
 * Shapes: epn_inter_c1_ok (cin = 1, no dense inter_w, cout in {16, 32, 48, 64}, ks <= 32); EPN_EINVAL otherwise.
 * Forward, ks = 24, even na, cout in {16, 32, 64}, nn <= 128: when the features do not depend on the anchor (checked on
 * the device, no host synchronisation; true for the occupancy feature) the relu arguments come off the matrix pipe
 * (inter_c1_fwd_mfma_kernel: rank-5 product, operands split without loss into 3 x bf16), otherwise -- or with
 * EPN_C1_MFMA=0 -- from the VALU kernel.  Outputs of the two agree to ~2e-6 of the tensor maximum.  The weight gradient
 * equals epn_gemm_tn_split_f32(grad_out rows, grouped), which is what the Python host calls (3-5x faster; EPN_C1_DW). */
int epn_inter_c1_ok(const epn_inter_desc *d);
int epn_inter_so3conv_fwd_c1_f32(const epn_inter_desc *d, const float *feats_cl, const float *W, float *out_cl,
                                 float *grouped, void *workspace, size_t workspace_bytes, epn_stream_t stream);
int epn_inter_so3conv_bwd_weight_c1_f32(const epn_inter_desc *d, const float *grouped, const float *grad_out_cl,
                                        float *grad_W, epn_stream_t stream);

/* 1 when the fused MFMA kernels serve this descriptor, 0 when the generic kernels do. */
int epn_inter_is_fused(const epn_inter_desc *d);

/* Materialise the weights for API compatibility (InterSO3Conv returns inter_w):
 * w f32[b,p2,na,ks,nn], formula of vgtk/vgtk/so3conv/functional.py:190-200. */
int epn_inter_weights_f32(const epn_inter_desc *d, float *w, epn_stream_t stream);

/* ------------------------------------------------------------------ IntraSO3Conv ------------ */

/* Replaces IntraSO3Conv.forward's compute (vgtk/vgtk/so3conv/modules.py:197-200 =
 * intra_so3conv_grouping (functional.py:221-233) -> BasicSO3Conv):
 *   out_cl[b,p,a,o] = sum_{c,k} W[o, c*kn+k] * feats_cl[b, p, intra_idx[a,k], c]
 * feats_cl f32[b,p,na,cin], intra_idx i32[na,kn], W f32[cout, cin*kn] -> out_cl f32[b,p,na,cout]. */
size_t epn_intra_workspace_bytes(int na, int kn, int cin, int cout);
int epn_intra_is_fused(int na, int kn, int cin, int cout);

int epn_intra_so3conv_fwd_f32(const float *feats_cl, const int32_t *intra_idx, const float *W,
                              int b, int p, int na, int kn, int cin, int cout, float *out_cl,
                              void *workspace, size_t workspace_bytes, epn_stream_t stream);

/* Autograd transposes.  `inv_idx` i32[na,kn] (optional) is the column-wise inverse of intra_idx,
 * inv_idx[intra_idx[a,k], k] = a; it exists when every column of intra_idx is a permutation of the
 * anchors (true for the icosahedral table) and makes the data gradient an atomic-free gather.  With
 * inv_idx == NULL a scatter-add kernel is used.  grad_feats_cl / grad_W are fully overwritten. */
int epn_intra_so3conv_bwd_data_f32(const float *grad_out_cl, const int32_t *intra_idx,
                                   const int32_t *inv_idx, const float *W, int b, int p, int na,
                                   int kn, int cin, int cout, float *grad_feats_cl, void *workspace,
                                   size_t workspace_bytes, epn_stream_t stream);
int epn_intra_so3conv_bwd_weight_f32(const float *feats_cl, const float *grad_out_cl,
                                     const int32_t *intra_idx, int b, int p, int na, int kn,
                                     int cin, int cout, float *grad_W, epn_stream_t stream);

/* ------------------------------------------------------------------ block glue ---- */

/* Normalisation + leaky_relu of SeparableSO3ConvBlock (SPConvNets/utils/base_so3conv.py:116-126, 52-62, 208-211:
 * `relu(norm(x))` with norm = BatchNorm2d or InstanceNorm2d(affine=False), relu = F.leaky_relu) on channels-last
 * tensors, as two memory-bound passes instead of torch's 4-6 (+ layout copies).  x_cl f32[groups][rows][c]:
 *   BatchNorm2d   : groups = 1, rows = b*p*a  (statistics per channel over every other axis)
 *   InstanceNorm2d: groups = b, rows = p*a    (statistics per (sample, channel))
 * sums f32[groups][c][2] = (sum x, sum x^2) is produced by epn_chan_stats_f32 (block partials in the workspace, then a
 * small finishing kernel: no atomics, deterministic) and consumed by the
 * apply passes: mean = s1/rows, var = s2/rows - mean^2 (biased, as both torch norms use for normalisation).
 *   y = leaky(((x - mean) * rsqrt(var + eps)) * gamma + beta, slope) (+ residual)      gamma/beta/residual optional
 * Backward: dsums f32[groups][c][2] = (sum dn, sum dn*xhat) with dn = dy * leaky'(.) * gamma, from
 * epn_norm_act_bwd_reduce_f32 (also writes dgamma / dbeta when given), then
 *   dx = rstd * (dn - mean(dn) - xhat * mean(dn * xhat))                               epn_norm_act_bwd_apply_f32 */
/* Scratch of the two reduction entry points: one (s1, s2) pair per block and channel,
 *   bytes = groups * blocks * c * 8,   blocks = ceil(rows / rows_per_block),
 *   rows_per_block = max(64, ceil(rows / ceil(1024 / groups)))
 * (about 1024 blocks in total, never fewer than 64 rows each); 0 for a c the kernels do not take (c / 4 must be a power of two
 * no greater than 256), groups > 65535, groups == 0 or rows == 0. */
size_t epn_norm_workspace_bytes(int groups, long long rows, int c);
/* BatchNorm2d's running statistics (training mode) from sums[c][2] of `count` values per channel, in one launch:
 * mean (+ conv_bias, the bias of the producing convolution when it was not added to x), unbiased variance,
 * num_batches_tracked += 1, running = running + momentum * (batch - running); momentum < 0 = None (cumulative average,
 * 1 / num_batches_tracked).  Reference: torch.nn.BatchNorm2d inside SeparableSO3ConvBlock (base_so3conv.py:168-212). */
int epn_bn_running_update_f32(const float *sums, double count, const float *conv_bias, float *running_mean,
                              float *running_var, long long *num_batches_tracked, float momentum, int c,
                              epn_stream_t stream);
int epn_chan_stats_f32(const float *x_cl, int groups, long long rows, int c, float *sums, void *workspace,
                       size_t workspace_bytes, epn_stream_t stream);
int epn_norm_act_fwd_f32(const float *x_cl, int groups, long long rows, int c, const float *sums,
                         const float *gamma, const float *beta, const float *residual_cl, float eps, float slope,
                         float *y_cl, epn_stream_t stream);
int epn_norm_act_bwd_reduce_f32(const float *x_cl, const float *dy_cl, int groups, long long rows, int c,
                                const float *sums, const float *gamma, const float *beta, float eps, float slope,
                                float *dsums, float *dgamma, float *dbeta, void *workspace,
                                size_t workspace_bytes, epn_stream_t stream);
int epn_norm_act_bwd_apply_f32(const float *x_cl, const float *dy_cl, int groups, long long rows, int c,
                               const float *sums, const float *dsums, const float *gamma, const float *beta,
                               float eps, float slope, float *dx_cl, epn_stream_t stream);

/* The tail of a SeparableSO3ConvBlock in one pass per direction (SPConvNets/utils/base_so3conv.py:204-211):
 *   y = leaky_relu(norm_a(xa)) + leaky_relu(norm_b(xb))
 * xa = the IntraSO3Conv output with its InstanceNorm2d, xb = the skip branch's 1x1 convolution with the block's norm.  The
 * skip branch's normalised tensor is never written; the backward passes read the common output gradient once.  Tensors are
 * [b clouds][rows per cloud][c] (float, or __bf16 with bf16 = 1; c % 4 == 0, 256 % (c/4) == 0).  A side is "instance"
 * (sums / dsums [b][c][2], statistics per cloud) or batch (sums / dsums [1][c][2] over all clouds); sums come from
 * epn_chan_stats_*.  bwd_reduce also writes dgamma / dbeta of a side when given; dx of a side may be NULL in bwd_apply. */
typedef struct epn_norm_pair_side {
    const float *sums;      /* [b or 1][c][2]: (sum x, sum x^2) */
    const float *gamma;     /* [c] or NULL */
    const float *beta;      /* [c] or NULL */
    float eps;
    int instance;           /* 1: statistics per cloud (InstanceNorm2d), 0: one set (BatchNorm2d) */
} epn_norm_pair_side;
size_t epn_norm_pair_workspace_bytes(int b, long long rows, int c);
int epn_norm_act_pair_fwd(const void *xa_cl, const void *xb_cl, int b, long long rows, int c,
                          const epn_norm_pair_side *side_a, const epn_norm_pair_side *side_b, float slope, void *y_cl,
                          int bf16, epn_stream_t stream);
int epn_norm_act_pair_bwd_reduce(const void *xa_cl, const void *xb_cl, const void *dy_cl, int b, long long rows, int c,
                                 const epn_norm_pair_side *side_a, const epn_norm_pair_side *side_b, float slope,
                                 float *dsums_a, float *dgamma_a, float *dbeta_a, float *dsums_b, float *dgamma_b,
                                 float *dbeta_b, void *workspace, size_t workspace_bytes, int bf16, epn_stream_t stream);
int epn_norm_act_pair_bwd_apply(const void *xa_cl, const void *xb_cl, const void *dy_cl, int b, long long rows, int c,
                                const epn_norm_pair_side *side_a, const epn_norm_pair_side *side_b, float slope,
                                const float *dsums_a, const float *dsums_b, void *dxa_cl, void *dxb_cl, int bf16,
                                epn_stream_t stream);

/* fp32 variants of three of the passes above that also write max |output| (of y / of dx / of side b's dx) into a device
 * scalar, zeroed by the call: the producer-side maxima of the two-piece fp16 GEMMs that consume those tensors (see
 * epn_gemm_nt_f16x2_f32).  bf16 = 1: EPN_EINVAL. */
int epn_norm_act_pair_fwd_amax(const void *xa_cl, const void *xb_cl, int b, long long rows, int c,
                               const epn_norm_pair_side *side_a, const epn_norm_pair_side *side_b, float slope, void *y_cl,
                               int bf16, float *y_amax, epn_stream_t stream);
int epn_norm_act_pair_bwd_apply_amax(const void *xa_cl, const void *xb_cl, const void *dy_cl, int b, long long rows, int c,
                                     const epn_norm_pair_side *side_a, const epn_norm_pair_side *side_b, float slope,
                                     const float *dsums_a, const float *dsums_b, void *dxa_cl, void *dxb_cl, int bf16,
                                     float *dxb_amax, epn_stream_t stream);
int epn_norm_act_bwd_apply_amax_f32(const float *x_cl, const float *dy_cl, int groups, long long rows, int c,
                                    const float *sums, const float *dsums, const float *gamma, const float *beta, float eps,
                                    float slope, float *dx_cl, float *dx_amax, epn_stream_t stream);

/* Dropout inside the norm passes: the nn.Dropout that follows norm + leaky_relu in every block of the reference
 * (SPConvNets/utils/base_so3conv.py:58-59 / 124-125; the separable block adds its skip branch after it, :205-211), as one
 * more multiply in passes that already stream the tensor.  The mask is not stored: it is a function of
 * (seed, call, e, rate) alone, e = the element's flat offset in the channels-last tensor (for logical [b][c][p][a]:
 * e = ((b_i*p + p_i)*a + a_i)*c + ch).  Element e is DROPPED iff
 *   Philox4x32-10(counter = {lo32(e>>2), hi32(e>>2), lo32(call), hi32(call)}, key = {lo32(seed), hi32(seed)})[e & 3]
 *       < floor(rate * 2^32)
 * (Salmon et al., SC'11: multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, 10 rounds), kept
 * elements are scaled by 1 / (1 - rate) (one fp32 division).  0 < rate < 1, else EPN_EINVAL.
 * state: DEVICE int64[2] = (seed, call), read by the kernels -- nothing of it is a launch argument, so a captured graph
 * draws a new mask on every replay.  epn_dropout_state_next copies state to `saved` (what the backward entry points of
 * that forward take as their `state`) and adds 1 to call.
 *   fwd       : y = m * leaky(norm(x)) / (1 - rate) (+ residual: added after the mask, never masked)
 *   bwd_reduce, bwd_apply: as the plain entry points with dy * m / (1 - rate) in place of dy (m regenerated); the
 *               residual's gradient is the caller's dy itself.
 * epn_dropout_mask_u8 writes the mask of `numel` elements from offset 0, one byte each, 1 = kept (mask 4-byte aligned). */
int epn_norm_act_dropout_fwd_f32(const float *x_cl, int groups, long long rows, int c, const float *sums,
                                 const float *gamma, const float *beta, const float *residual_cl, float eps, float slope,
                                 double rate, const long long *state, float *y_cl, epn_stream_t stream);
int epn_norm_act_dropout_bwd_reduce_f32(const float *x_cl, const float *dy_cl, int groups, long long rows, int c,
                                        const float *sums, const float *gamma, const float *beta, float eps, float slope,
                                        double rate, const long long *state, float *dsums, float *dgamma, float *dbeta,
                                        void *workspace, size_t workspace_bytes, epn_stream_t stream);
int epn_norm_act_dropout_bwd_apply_f32(const float *x_cl, const float *dy_cl, int groups, long long rows, int c,
                                       const float *sums, const float *dsums, const float *gamma, const float *beta,
                                       float eps, float slope, double rate, const long long *state, float *dx_cl,
                                       epn_stream_t stream);
/* bf16 features (x / y / dy / dx / residual are __bf16; statistics, parameters and arithmetic fp32), same reference lines
 * (base_so3conv.py:58-59 / 124-125) */
int epn_norm_act_dropout_fwd_bf16(const void *x_cl, int groups, long long rows, int c, const float *sums,
                                  const float *gamma, const float *beta, const void *residual_cl, float eps, float slope,
                                  double rate, const long long *state, void *y_cl, epn_stream_t stream);
int epn_norm_act_dropout_bwd_reduce_bf16(const void *x_cl, const void *dy_cl, int groups, long long rows, int c,
                                         const float *sums, const float *gamma, const float *beta, float eps, float slope,
                                         double rate, const long long *state, float *dsums, float *dgamma, float *dbeta,
                                         void *workspace, size_t workspace_bytes, epn_stream_t stream);
int epn_norm_act_dropout_bwd_apply_bf16(const void *x_cl, const void *dy_cl, int groups, long long rows, int c,
                                        const float *sums, const float *dsums, const float *gamma, const float *beta,
                                        float eps, float slope, double rate, const long long *state, void *dx_cl,
                                        epn_stream_t stream);
int epn_dropout_mask_u8(unsigned char *mask, long long numel, double rate, const long long *state, epn_stream_t stream);
int epn_dropout_state_next(long long *state, long long *saved, epn_stream_t stream);

/* Frozen statistics: the forward passes above for a network in eval() mode, where torch.nn.BatchNorm2d normalises with its
 * running statistics instead of the batch's (forward only: no backward forms, no running-statistics update, no maximum
 * variants -- a consumer that needs max |y| scans the tensor).  Every pass reads stats f32[c][2] = (mean, var) AS THEY ARE,
 * rstd = rsqrt(var + eps), one group: the statistics are never turned into (sum x, sum x^2) for the entry points above,
 * because var = s2 / rows - mean^2 cancels when mean^2 >> var.  Sizes as their twins: c % 4 == 0, 256 % (c / 4) == 0.
 *
 * epn_bn_frozen_stats_f32 writes stats_out[c][2] = (running_mean - conv_bias, running_var) in one launch, reading through the
 * pointers (no host synchronisation: an eval forward can be captured in a graph, and a replay follows statistics changed in
 * place).  conv_bias (or NULL): the bias of the producing convolution when it was NOT added to x.  Batch statistics cancel such
 * a bias, running statistics do not: y = (x + b - running_mean) * rstd * gamma + beta.  Replaces torch.nn.BatchNorm2d in eval
 * mode inside SeparableSO3ConvBlock / InterSO3ConvBlock / ClsOutBlockPointnet (base_so3conv.py:168-212 / :87-126 / :358-448). */
int epn_bn_frozen_stats_f32(const float *running_mean, const float *running_var, const float *conv_bias, int c,
                            float *stats_out, epn_stream_t stream);
/* y = leaky((x - mean) * rsqrt(var + eps) * gamma + beta, slope) (+ residual); x_cl [rows][c], rows = b*p*a; gamma / beta /
 * residual optional.  The twin of epn_norm_act_fwd_*; replaces relu(torch.nn.BatchNorm2d(x)) in eval mode
 * (base_so3conv.py:168-212 / :87-126, and with slope = 0 the head's mlp, :358-448). */
int epn_norm_act_frozen_fwd_f32(const float *x_cl, long long rows, int c, const float *stats, const float *gamma,
                                const float *beta, const float *residual_cl, float eps, float slope, float *y_cl,
                                epn_stream_t stream);
int epn_norm_act_frozen_fwd_bf16(const void *x_cl, long long rows, int c, const float *stats, const float *gamma,
                                 const float *beta, const void *residual_cl, float eps, float slope, void *y_cl,
                                 epn_stream_t stream);
/* The twin of epn_norm_act_pair_fwd: y = leaky_relu(norm_a(xa)) + leaky_relu(norm_b(xb)) with side a as there (statistics
 * from its sums) and side b either frozen (stats[c][2] = (mean, var): torch.nn.BatchNorm2d in eval mode on the skip branch,
 * base_so3conv.py:168-212) or instance (stats = sums[b][c][2] per cloud, as an "instance" epn_norm_pair_side). */
typedef struct epn_norm_pair_frozen_side {
    const float *stats;     /* frozen: [c][2] = (mean, var);  else [b][c][2] = (sum x, sum x^2) per cloud */
    const float *gamma;     /* [c] or NULL */
    const float *beta;      /* [c] or NULL */
    float eps;
    int frozen;             /* 1: frozen statistics, 0: instance statistics from sums */
} epn_norm_pair_frozen_side;
int epn_norm_act_pair_frozen_fwd(const void *xa_cl, const void *xb_cl, int b, long long rows, int c,
                                 const epn_norm_pair_side *side_a, const epn_norm_pair_frozen_side *side_b, float slope,
                                 void *y_cl, int bf16, epn_stream_t stream);

/* replaces vgtk.cuda.grouping.initial_anchor_query (vgtk/vgtk/cuda/grouping_cuda.cpp:138-158, kernel
 * grouping_cuda_kernel.cu:116-167; only consumer: KernelPropagation, vgtk/vgtk/so3conv/modules.py:57-119).
 *   centers f32[b][3][nc]   xyz f32[m][3] (fragment points, shared by the batch)   kernel_points f32[ks][na][3]
 *   anchor_weights f32[b][ks][nc][na] = sum over fragment points within `radius` of the centre (sqrt distance, <=) of
 *                                       max(1 - |centre + kernel_point - x|^2 / sigma, 0)
 *   anchor_ctn     f32[b][ks][nc][na] = number of such points (same value for every ks, na)
 * Both outputs are fully written (the reference zero-fills and accumulates with atomics, and reads xyz[3*pm] past the
 * end for its padding threads; neither is reproduced).  ks*na <= 2048. */
int epn_initial_anchor_query_f32(const float *centers, const float *xyz, const float *kernel_points, int b, int nc,
                                 int m, int na, int ks, float radius, float sigma, float *anchor_weights,
                                 float *anchor_ctn, epn_stream_t stream);
/* the scalar_t = double instantiation of the same kernel (AT_DISPATCH_FLOATING_TYPES on xyz.type(),
 * grouping_cuda_kernel.cu:558-563; outputs take the inputs' dtype, grouping_cuda.cpp:149-154).  radius and sigma stay
 * FLOAT parameters as in the reference (:127-128) and are widened where they meet a double. */
int epn_initial_anchor_query_f64(const double *centers, const double *xyz, const double *kernel_points, int b, int nc,
                                 int m, int na, int ks, float radius, float sigma, double *anchor_weights,
                                 double *anchor_ctn, epn_stream_t stream);

/* InterSO3Conv with the grouped features kept ON CHIP (north_star: "the [B,N,K,A,C] tile staged through LDS"): the same
 * result as epn_inter_so3conv_fwd_f32 -- vgtk/vgtk/so3conv/modules.py:157-174 = inter_so3conv_grouping
 * (vgtk/vgtk/spconv/functional.py:372-390) -> BasicSO3Conv (modules.py:48-55) -- with the neighbour contraction as the
 * A-tile producer of the weight contraction; no [cols, cin*ks] tensor is written.
 *   _onchip_f32: fp32 features / output; the weight contraction runs on the bf16 matrix pipe with both operands split
 *                losslessly into three bf16 pieces (as epn_gemm_nt_split_f32: fp32 accuracy; non-finite inputs give NaN).
 *   _bf16:       bf16 features / output ("bf16 features, fp32 accumulate"), W fp32 master weights (rounded per call).
 * Shapes served: epn_inter_onchip_ok(d, bf16) != 0 (cin % 16 == 0, cout % 32 == 0, cout <= 256, ks in {16, 24},
 * nn <= 64, 32 < na <= 64, no dense_w); EPN_EINVAL otherwise.  Workspace: epn_inter_onchip_workspace_bytes. */
int epn_inter_onchip_ok(const epn_inter_desc *d, int bf16);
size_t epn_inter_onchip_workspace_bytes(const epn_inter_desc *d, int bf16);
int epn_inter_so3conv_fwd_onchip_f32(const epn_inter_desc *d, const float *feats_cl, const float *W, float *out_cl,
                                     void *workspace, size_t workspace_bytes, epn_stream_t stream);
int epn_inter_so3conv_fwd_bf16(const epn_inter_desc *d, const void *feats_cl, const float *W, void *out_cl,
                               void *workspace, size_t workspace_bytes, epn_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * Grouping only ("split" convolution): the grouped features as a tensor, the weight contraction left to the caller's
 * BLAS.  replaces vgtk/vgtk/so3conv/functional.py:118-140 (inter_so3conv_grouping: ball grouping + anchor weights +
 * inter_zpconv_grouping_naive, vgtk/vgtk/spconv/functional.py:372-421) and its autograd backward; what follows it in the
 * reference, BasicSO3Conv.forward (vgtk/vgtk/so3conv/modules.py:38-52: W @ feats.view(b, c*ks, p*a)), stays a matmul.
 *   grouped f32[b*p2*na][cin*ks]   row = column (b, p, a), element c*ks + k  -- the reference's [b, c, ks, p2, na] tensor
 *                                  with the (c, ks) axes last, so  out_cl[col][o] = grouped[col][:] . W[o][:]
 * epn_inter_ungroup_f32 is the transpose: grad_feats_cl[b][idx][a][c] += sum_k w * grad_grouped (zero-fills first).
 * Its workgroups take 8-16 output points that are neighbours in space (Morton order of new_xyz, computed into the
 * workspace), sum the contributions of the slots that name the same input point in LDS and issue one fp32 atomic per
 * distinct (input point, anchor, channel): ~3x fewer atomics than one per slot.
 * cout / dense_w of the descriptor are ignored (dense_w must be NULL).  Neither inter_w nor the gathered neighbour
 * features are materialised; the fused entry points above additionally avoid `grouped` itself (inference, or when
 * HBM is short: `grouped` is cin*ks*4 bytes per column, 6 GB for a 64-channel layer at B=32). */
size_t epn_inter_group_workspace_bytes(const epn_inter_desc *d);
int epn_inter_group_f32(const epn_inter_desc *d, const float *feats_cl, float *grouped, void *workspace,
                        size_t workspace_bytes, epn_stream_t stream);
int epn_inter_ungroup_f32(const epn_inter_desc *d, const float *grad_grouped, float *grad_feats_cl, void *workspace,
                          size_t workspace_bytes, epn_stream_t stream);
/* epn_inter_ungroup_acc_{f32,bf16}: the same transpose ADDED to the contents of grad_feats_cl (fp32) instead of written
 * over zeros -- for a tensor whose gradient also arrives by another path (the input of a SeparableSO3ConvBlock feeds the
 * inter convolution AND the skip branch, base_so3conv.py:186-207): hand in the other path's gradient and neither a
 * zero-fill nor a separate addition pass is needed. */
int epn_inter_ungroup_acc_f32(const epn_inter_desc *d, const float *grad_grouped, float *grad_feats_cl, void *workspace,
                              size_t workspace_bytes, epn_stream_t stream);
int epn_inter_ungroup_acc_bf16(const epn_inter_desc *d, const void *grad_grouped, float *grad_feats_cl, void *workspace,
                               size_t workspace_bytes, epn_stream_t stream);

/* Packed column order of `grouped` (what the split convolution of this package uses between its own kernels).  In the
 * element order c*ks + k above, one store instruction of the grouping kernel -- four kernel points of 16 channels -- is 16
 * pieces of 64 (or 32) bytes, ks*4 bytes or more apart; the kernel is bound by those stores (6 GB per 64-channel layer at
 * B=32).  In the packed order every store instruction covers one contiguous 1 KiB / 512 B range of the row: 8-20 % less
 * kernel time.  A matrix product does not care about the order of its contraction index as long as both operands agree, so
 * the WEIGHTS are permuted instead (a few MB): same result as the plain order bit for bit up to summation order.
 *   epn_inter_packed_position(cin, ks, position[cin*ks]) : host table, position[c*ks + k] = column of element (c, k):
 *       CG = 4 if cin % 64 == 0 else 2;  slot(c) = c - c % (16 CG) + 16 (c % CG) + (c % (16 CG)) / CG;
 *       k < 16:  slot * min(ks, 16) + k;   k >= 16:  min(ks, 16) * cin + slot * (ks - 16) + (k - 16)
 *   epn_inter_group_packed_{f32,bf16} : as epn_inter_group_*, columns in packed order; shapes: epn_inter_group_packed_ok
 *       (the MFMA grouping kernel's shapes with na >= 16, cin % 32 == 0, nn <= 64), EPN_EINVAL otherwise
 *   epn_inter_pack_weights_{f32,bf16} : packed[o][position[q]] = W[o][q]   (fp32 master weights -> fp32 / bf16 operand)
 *   epn_inter_unpack_weight_grad_f32  : grad_W[o][q] = grad_packed[o][position[q]]   (gradient computed against packed G)
 * The gradient of `grouped` stays in the plain order (epn_inter_ungroup_*: its reads are not what bounds that kernel). */
int epn_inter_group_packed_ok(const epn_inter_desc *d);
int epn_inter_packed_position(int cin, int ks, int32_t *position);
int epn_inter_group_packed_f32(const epn_inter_desc *d, const float *feats_cl, float *grouped, void *workspace,
                               size_t workspace_bytes, epn_stream_t stream);
int epn_inter_group_packed_bf16(const epn_inter_desc *d, const void *feats_cl, void *grouped, void *workspace,
                                size_t workspace_bytes, epn_stream_t stream);
int epn_inter_pack_weights_f32(const float *W, int cout, int cin, int ks, float *packed, epn_stream_t stream);
int epn_inter_pack_weights_bf16(const float *W, int cout, int cin, int ks, void *packed, epn_stream_t stream);
int epn_inter_unpack_weight_grad_f32(const float *grad_packed, int cout, int cin, int ks, float *grad_W,
                                     epn_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * Composed split form: InterSO3Conv forward / backward as ONE call per direction on the kernel chain the benchmark times
 * replaces InterSO3Conv.forward (vgtk/vgtk/so3conv/modules.py:157-174: L.inter_so3conv_grouping, so3conv/functional.py:118-178,
 * then BasicSO3Conv's matmul, modules.py:48-55) and the autograd transposes of both -- the same boundary as
 * epn_inter_so3conv_{fwd,bwd_data,bwd_weight}_f32 above (the fused fp32-MFMA kernels), but running
 *   forward : epn_inter_group_packed_* (plain order where the packed one does not apply) -> epn_inter_pack_weights_* ->
 *             epn_gemm_nt_split_f32 (fp32: lossless 3 x bf16 split, fp32 accuracy) / epn_gemm_nt_bf16
 *   backward: epn_gemm_tn_split_f32 / _bf16 (+ epn_inter_unpack_weight_grad_f32) for grad_W;
 *             epn_transpose_cast -> epn_gemm_nt_* -> epn_inter_ungroup[_acc]_* for grad_feats
 * i.e. exactly what epn_pointcloud_amd/ops.py's InterSO3ConvSplitFn issues; a binding of the reference's four-call surface
 * (grouping_cuda.cpp:176-181 + the two matmul gradients) gets the benchmarked path.  Buffers are the caller's:
 *   saved     : the grouped features G[b*p2*na][cin*ks] (feature dtype) written by forward and read by backward --
 *               epn_inter_split_saved_bytes(d, bf16); column order is an implementation detail of the pair
 *   workspace : scratch of one call -- epn_inter_split_workspace_bytes(d, bf16, backward_pass); the backward scratch holds
 *               the gradient of the grouped features (same size as `saved`)
 *   out_col_stats (optional, NULL: off): per-32-row-block column statistics of out_cl, see epn_gemm_nt_problem::col_stats
 *   backward: grad_feats_cl (fp32 scatter target for either feature dtype; NULL: not wanted; accumulate != 0: ADD to its
 *             contents, see epn_inter_ungroup_acc_*), grad_W f32[cout][cin*ks] (NULL: not wanted).
 * Shapes: the MFMA grouping kernels' (no dense inter_w, cin % 16 == 0, ks % 4 == 0, ks <= 32, nn <= 128) -- epn_inter_split_ok;
 * EPN_EINVAL otherwise (use the fused entry points).  feats_cl / out_cl / grad_out_cl are float (…_f32) or bf16 (…_bf16);
 * W and grad_W are always fp32 (master weights). */
int epn_inter_split_ok(const epn_inter_desc *d);
size_t epn_inter_split_saved_bytes(const epn_inter_desc *d, int bf16);
size_t epn_inter_split_workspace_bytes(const epn_inter_desc *d, int bf16, int backward_pass);
int epn_inter_so3conv_fwd_split_f32(const epn_inter_desc *d, const float *feats_cl, const float *W, float *out_cl,
                                    float *out_col_stats, void *saved, size_t saved_bytes, void *workspace,
                                    size_t workspace_bytes, epn_stream_t stream);
int epn_inter_so3conv_fwd_split_bf16(const epn_inter_desc *d, const void *feats_cl, const float *W, void *out_cl,
                                     float *out_col_stats, void *saved, size_t saved_bytes, void *workspace,
                                     size_t workspace_bytes, epn_stream_t stream);
int epn_inter_so3conv_bwd_split_f32(const epn_inter_desc *d, const float *grad_out_cl, const float *W, const void *saved,
                                    size_t saved_bytes, float *grad_feats_cl, int accumulate, float *grad_W,
                                    void *workspace, size_t workspace_bytes, epn_stream_t stream);
int epn_inter_so3conv_bwd_split_bf16(const epn_inter_desc *d, const void *grad_out_cl, const float *W, const void *saved,
                                     size_t saved_bytes, float *grad_feats_cl, int accumulate, float *grad_W,
                                     void *workspace, size_t workspace_bytes, epn_stream_t stream);

/* IntraSO3Conv grouping as a tensor: replaces L.intra_so3conv_grouping (vgtk/vgtk/so3conv/functional.py:255-268,
 * feats[..., intra_idx]); IntraSO3Conv's BasicSO3Conv matmul (modules.py:197-200) then runs on the caller's BLAS.
 *   grouped f32[b*p*na][kn*c]   element k*c + ci = feats_cl[b][p][intra_idx[a][k]][ci]   (anchor-neighbour major, so
 *   the matching weight is W[o][ci*kn + k] re-ordered to [o][k*c + ci]; the reference tensor is [b, c, kn, p, na]).
 * Its transpose is the same gather through the inverse permutation (epn_intra_so3conv_bwd_data_f32 covers it fused). */
int epn_intra_group_f32(const float *feats_cl, const int32_t *intra_idx, float *grouped, int b, int p, int na, int kn,
                        int c, epn_stream_t stream);

/* Change of anchor basis for the block-diagonal form of IntraSO3Conv (epn_pointcloud_amd/so3_fourier.py): the twelve
 * anchor permutations of L.intra_so3conv_grouping (vgtk/vgtk/so3conv/functional.py:255-268) are simultaneously
 * block-diagonalised by one orthogonal matrix U, so IntraSO3Conv.forward (modules.py:197-200) becomes: U^T, one GEMM per
 * irreducible block, U -- 2.95x fewer flops than the 12-neighbour contraction and no grouped tensor.
 *   out[pt][r][ch] = sum_s M[r][s] * in[pt][s][ch]      M f32[na][na] row-major, pts points, c channels (c % 32 == 0)
 * `*_spectral` = 0: plain channels-last rows ((pt*na + r)*c);  1: row f of a point lives in its block's buffer at
 * ((blocks[f][0]*pts + pt*blocks[f][1] + (f - blocks[f][0]))*c), blocks i32[na][2] = (first row of the block, d*d), so
 * each block is a dense row-major [pts*d][d*c] matrix.  Forward transform: M = U^T, out_spectral = 1; inverse: M = U,
 * in_spectral = 1 (each is the other's transpose, i.e. its backward). */
int epn_so3_basis_f32(const float *in, const float *M, const int32_t *blocks, long long pts, int na, int c,
                      int in_spectral, int out_spectral, float *out, epn_stream_t stream);
/* The same transform (out_spectral must be 0) that also writes point_stats[pt][c][2] = (sum, sum of squares) over the na
 * output rows of every point, from the accumulators: the block partials (one block per point) of the per-channel statistics
 * of `out` for epn_stats_finish -- the InstanceNorm that follows IntraSO3Conv (base_so3conv.py:204-211) without a
 * statistics pass over `out`.  _split_f32: fp32 on the bf16 matrix pipe; _bf16: bf16 features (sums of the
 * rounded values). */
/* IntraSO3Conv's weights in the block-diagonal basis (so3_fourier.py): for every irreducible block rho (dimension d, first
 * spectral row `base`, blocks[f] = (base, d*d) as above) What^rho[(j, c), (i, o)] = sum_k W[o, c, k] R[base + i d + j][k],
 * R f32[na][kn] = the representation matrices rho(g_k)[i, j] of the kn anchor neighbours.  what: flat, block rho at offset
 * base * cin * cout as a row-major [d*cin][d*cout] matrix; what_t: the same blocks transposed ([d*cout][d*cin], the Bt
 * operand of epn_gemm_nt for the forward product); either may be NULL.  epn_spectral_weights_bwd_f32 is the transpose
 * (grad_W[o][c][k] from grad_what in the `what` layout).  Replaces nothing in the reference (the spectral form is this
 * library's); it replaces ~25 small torch launches per layer and direction.  A block dimension above 7 is NOT
 * supported: the kernels recover d from blocks[f][1] = d*d through a ladder that ends at 7 (1 + 9 + 9 + 16 + 25 of the
 * icosahedral group needs 5), and the entries do not check it. */
int epn_spectral_weights_f32(const float *W, const float *R, const int32_t *blocks, int cout, int cin, int kn, int na,
                             float *what, float *what_t, epn_stream_t stream);
/* the same blocks rounded to bf16 (fp32 master weights -> the operands of a bf16 network's GEMMs) */
int epn_spectral_weights_bf16(const float *W, const float *R, const int32_t *blocks, int cout, int cin, int kn, int na,
                              void *what, void *what_t, epn_stream_t stream);
int epn_spectral_weights_bwd_f32(const float *grad_what, const float *R, const int32_t *blocks, int cout, int cin, int kn,
                                 int na, float *grad_W, epn_stream_t stream);
int epn_so3_basis_stats_f32(const float *in, const float *M, const int32_t *blocks, long long pts, int na, int c,
                            int in_spectral, int out_spectral, float *out, float *point_stats, epn_stream_t stream);
int epn_so3_basis_stats_split_f32(const float *in, const float *M, const int32_t *blocks, long long pts, int na, int c,
                                  int in_spectral, int out_spectral, float *out, float *point_stats, epn_stream_t stream);
int epn_so3_basis_stats_bf16(const void *in, const float *M, const int32_t *blocks, long long pts, int na, int c,
                             int in_spectral, int out_spectral, void *out, float *point_stats, epn_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * PointnetSO3Conv: the aggregation tail of every shipped model
 * replaces vgtk/vgtk/so3conv/modules.py:203-235 (PointnetSO3Conv.forward: centre xyz, rotate it into every anchor frame
 * with einsum 'aji,bjn->bina', concatenate to the features, 1x1 Conv2d "embed", torch.max over the point axis) -- one
 * fused pass, neither the concatenated tensor nor the per-point embedding is written to HBM.
 *   feats_cl f32[b][p][a][c]   channels-last features          xyz   f32[b][3][p]
 *   anchors  f32[a][3][3] or NULL (a == 1: no rotation, modules.py:227-228)
 *   W        f32[co][c+3]      embed.weight (feature channels first, then the 3 coordinates)     bias f32[co] or NULL
 *   out      f32[b][a][co]     = logical [b, co, a] viewed channels-last
 *   argmax   i32[b][a][co]     point index of the maximum (first maximum wins), consumed by the backward entry points
 *   centre   f32[b][3]         per-cloud mean of xyz, consumed by epn_pointnet_so3conv_bwd_weight_f32
 * Backward = torch.max backward composed with the 1x1 convolution: gradients flow through the arg-max point only.
 * xyz receives no gradient (the reference never asks for one: coordinates are inputs). */
int epn_pointnet_so3conv_fwd_f32(const float *feats_cl, const float *xyz, const float *anchors, const float *W,
                                 const float *bias, float *out, int32_t *argmax, float *centre, int b, int p, int a,
                                 int c, int co, epn_stream_t stream);
int epn_pointnet_so3conv_bwd_data_f32(const float *grad_out, const int32_t *argmax, const float *W,
                                      float *grad_feats_cl, int b, int p, int a, int c, int co, epn_stream_t stream);
int epn_pointnet_so3conv_bwd_weight_f32(const float *grad_out, const int32_t *argmax, const float *feats_cl,
                                        const float *xyz, const float *anchors, const float *centre, float *grad_W,
                                        float *grad_bias, int b, int p, int a, int c, int co, epn_stream_t stream);

/* PointnetSO3Conv composed with the library's GEMMs (same module, vgtk/vgtk/so3conv/modules.py:219-235; the form the
 * benchmarked networks run for c % 16 == 0): the caller forms the embedding's feature part with epn_gemm_nt_*
 *     Z[b][p][a][o] = sum_c W[o][c] F[b][p][a][c]          (rows = the channels-last feature rows; fp32 result)
 * and these entries do the rest.
 *   epn_pointnet_max_f32:  out[b][a][o] = max_p (Z + sum_j W[o][c+j] ext_j[b][p][a] + bias[o]), argmax = first maximum,
 *                          centre[b][3] = mean_p xyz (ext = R_a^T (xyz - centre); anchors NULL: identity).  W is the
 *                          full [co][c+3] weight, of which only the three coordinate columns are read.
 *   epn_pointnet_dz_*:     dZ[b][p][a][o] = argmax[b][a][o] == p ? grad_out[b][a][o] : 0 (every element written;
 *                          co % 8 == 0, 16-byte aligned pointers) -- then dF = dZ W (epn_gemm_nt_*), dW[:, :c] = dZ^T F
 *                          (epn_gemm_tn_*).  _bf16: dZ in bf16 for bf16 features.
 *   epn_pointnet_bwd_coord_f32: grad_W[o][c + j] = sum_{b,a} grad_out ext_j[b][argmax][a] (the other columns of the
 *                          [co][c+3] buffer are not touched), grad_bias[o] = sum_{b,a} grad_out (may be NULL); fixed
 *                          summation order. */
int epn_pointnet_max_f32(const float *Z, const float *xyz, const float *anchors, const float *W, const float *bias,
                         float *out, int32_t *argmax, float *centre, int b, int p, int a, int c, int co,
                         epn_stream_t stream);
int epn_pointnet_dz_f32(const float *grad_out, const int32_t *argmax, float *dZ, int b, int p, int a, int co,
                        epn_stream_t stream);
int epn_pointnet_dz_bf16(const float *grad_out, const int32_t *argmax, void *dZ, int b, int p, int a, int co,
                         epn_stream_t stream);
int epn_pointnet_bwd_coord_f32(const float *grad_out, const int32_t *argmax, const float *xyz, const float *anchors,
                               const float *centre, float *grad_W, float *grad_bias, int b, int p, int a, int c, int co,
                               epn_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * vgtk.cuda.zpconv: grouping functions of the legacy ZPConv path (unreachable from the shipped models,
 * provided for API completeness).  Layouts are the reference's (channel-major, contiguous).
 * replaces inter_zpconv_forward / inter_zpconv_backward / intra_zpconv_forward / intra_zpconv_backward
 * (vgtk/vgtk/cuda/zpconv_cuda.cpp:41-112; kernels zpconv_cuda_kernel.cu:33-195).
 *   inter: anchor_neighbors i32[b][np][na][ks][ann], anchor_weights f32 (same shape), feats f32[b][c][nq][na]
 *          anchor_feats f32[b][c][ks][np][na] = sum_ni feats[b][c][nbr][a] * w      (forward: gather, no atomics)
 *          grad_feats   f32[b][c][nq][na]  (zero-filled here, fp32 atomic scatter)
 *   intra: anchor_neighbors i32[na_out][ann], anchor_weights f32[na_out][ks][ann], feats f32[b][c][np][na_in]
 *          anchor_feats f32[b][c][ks][np][na_out];  grad_feats f32[b][c][np][na_in]
 * Indices outside [0, nq) / [0, na_in) contribute nothing (the reference reads out of bounds). */
/* replaces vgtk.cuda.grouping.anchor_query (vgtk/vgtk/cuda/grouping_cuda.cpp:88-108, kernel
 * grouping_cuda_kernel.cu:180-247; legacy ZPConv, every call site in the reference is commented out):
 *   grouped_xyz f32[b][3][np][nn] (local coordinates), anchors f32[na][3] (unit directions), kernel_points f32[ks][2]
 *   anchor_weights f32[b][np][na][ks][nn] = (kw - norm)^2 + ((kh - theta) * norm)^2,
 *       norm = |g| + 1e-6, theta = acos(g . anchor / norm)      (fully written; the reference pre-fills 1e6)
 * The reference's sample_idx / grouped_indices / nq arguments are unused by its kernel and not part of this entry. */
int epn_anchor_query_f32(const float *grouped_xyz, const float *anchors, const float *kernel_points, int b, int np,
                         int nn, int na, int ks, float *anchor_weights, epn_stream_t stream);
/* scalar_t = double (grouping_cuda_kernel.cu:505-510; the output takes grouped_xyz's dtype, grouping_cuda.cpp:103-104).
 * In BOTH instantiations `+ 1e-6` adds a double literal (:221): the f32 entry forms |g| + 1e-6 in double and rounds
 * once. */
int epn_anchor_query_f64(const double *grouped_xyz, const double *anchors, const double *kernel_points, int b, int np,
                         int nn, int na, int ks, double *anchor_weights, epn_stream_t stream);
int epn_zp_inter_fwd_f32(const int32_t *anchor_neighbors, const float *anchor_weights, const float *feats, int b, int c,
                         int np, int nq, int na, int ks, int ann, float *anchor_feats, epn_stream_t stream);
int epn_zp_inter_bwd_f32(const int32_t *anchor_neighbors, const float *anchor_weights, const float *grad_anchor_feats,
                         int b, int c, int np, int nq, int na, int ks, int ann, float *grad_feats, epn_stream_t stream);
int epn_zp_intra_fwd_f32(const int32_t *anchor_neighbors, const float *anchor_weights, const float *feats, int b, int c,
                         int np, int na_in, int na_out, int ks, int ann, float *anchor_feats, epn_stream_t stream);
int epn_zp_intra_bwd_f32(const int32_t *anchor_neighbors, const float *anchor_weights, const float *grad_anchor_feats,
                         int b, int c, int np, int na_in, int na_out, int ks, int ann, float *grad_feats,
                         epn_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * BasicSO3Conv's weight contraction and its autograd transposes as hand-written MFMA GEMMs
 * replaces BasicSO3Conv.forward (vgtk/vgtk/so3conv/modules.py:48-55: `torch.matmul(self.W, x.view(b, c*ks, p*a))`) and
 * the two matmul gradients torch autograd derives from it.  Operands are row-major with explicit leading dimensions.
 *   NT: C[M][N]   = A[M][K] . Bt[N][K]^T   (activations x weights: out = grouped W^T, grad_grouped = grad_out (W^T)^T,
 *                                           the irreducible blocks of the spectral IntraSO3Conv); up to any number of
 *                                           problems per call (one grouped launch per 6).
 *   TN: C[N1][N2] = X[R][N1]^T . Y[R][N2]  (weight gradients: contraction over the R = b*p*a columns; split over R into
 *                                           fp32 partials in `workspace`, summed in a fixed order: deterministic).
 * fp32: v_mfma_f32_32x32x2_f32, exact f32 (the split entry points below: the bf16 pipe at fp32 accuracy).  bf16: bf16 operands, fp32 accumulation; NT writes bf16 (or fp32 when
 * out_f32 != 0), TN always writes fp32.  Fast path: K % 32 == 0 (fp32) / 64 (bf16), 16-byte aligned rows; anything
 * else runs on a generic kernel.  C is fully overwritten.  An NT problem with M == 0 is empty: nothing is read or written for
 * it, and its A and C may be NULL (Bt, N >= 1 and K >= 1 are still required); it may stand anywhere in a grouped call. */
typedef struct epn_gemm_nt_problem {
    const void *A, *Bt;
    void *C;
    long long M, lda, ldb, ldc;
    int N, K;
    /* Optional (NULL: off): per-column statistics of C taken from the accumulators in the kernel's epilogue --
     * col_stats[(m / 32)][n][2] = (sum, sum of squares) of rows 32 (m / 32) .. + 31 of column n, as stored (bf16 outputs:
     * of the rounded values); M % 32 == 0.  epn_stats_finish turns them into the sums[groups][N][2] the norm entry points
     * take: the per-channel statistics pass of a following BatchNorm / InstanceNorm (base_so3conv.py:196-204) without
     * reading C again. */
    float *col_stats;
    /* Optional (NULL: off; library 0.5): device scalar the kernel RAISES to max|C| (values as stored; non-finite ones left
     * out) from its accumulators -- zero it before the call.  What epn_inter_ungroup_cloud_* takes as dg_amax when C is the
     * gradient of the grouped features. */
    float *c_amax;
} epn_gemm_nt_problem;
int epn_gemm_nt_f32(int nprob, const epn_gemm_nt_problem *probs, epn_stream_t stream);
/* sums[g][c][2] = sum over the blocks_per_group consecutive 32-row blocks of group g of partials[block][c][2] (fixed
 * order: deterministic).  groups = 1 for BatchNorm2d, the number of clouds for InstanceNorm2d (rows per cloud % 32 == 0). */
/* Workspace: 0 up to 2048 blocks per group (one kernel); above, the blocks are first summed 256 at a time into
 * groups * ceil(blocks_per_group / 256) * c * 8 bytes. */
size_t epn_stats_finish_workspace_bytes(int groups, long long blocks_per_group, int c);
int epn_stats_finish(const float *partials, int groups, long long blocks_per_group, int c, float *sums, void *workspace,
                     size_t workspace_bytes, epn_stream_t stream);
int epn_gemm_nt_bf16(int nprob, const epn_gemm_nt_problem *probs, int out_f32, epn_stream_t stream);
/* Split form of the fp32 NT contraction: the same fp32 operands and fp32 result, computed on the bf16 matrix pipe.
 * Every fp32 value is split WITHOUT LOSS into three bf16 pieces (round-to-nearest remainders); the six piece products
 * of weight >= 2^-16 are accumulated in fp32, the three dropped ones are below 2^-24 |a||b| (less than the rounding
 * of one fp32 FMA): fp32 accuracy at 2.7x the matrix rate of v_mfma_f32_32x32x2_f32.  Bt (the weights) is split once
 * per call into `workspace` (epn_gemm_nt_split_workspace_bytes); problems that do not qualify (K % 32, row alignment)
 * or a missing workspace run on epn_gemm_nt_f32's kernels. */
size_t epn_gemm_nt_split_workspace_bytes(int nprob, const epn_gemm_nt_problem *probs);
int epn_gemm_nt_split_f32(int nprob, const epn_gemm_nt_problem *probs, void *workspace, size_t workspace_bytes,
                          epn_stream_t stream);
/* `bf16`: 0 = fp32 operands (epn_gemm_tn_f32), 1 = bf16 (epn_gemm_tn_bf16), 2 = fp32 operands in the split form
 * (epn_gemm_tn_split_f32: the partial slabs plus, for N2 >= 512, the three bf16 planes of X = 6 bytes per value) */
size_t epn_gemm_tn_workspace_bytes(int bf16, long long R, int N1, int N2);
int epn_gemm_tn_f32(const float *X, long long ldx, const float *Y, long long ldy, float *C, long long ldc, long long R,
                    int N1, int N2, void *workspace, size_t workspace_bytes, epn_stream_t stream);
int epn_gemm_tn_bf16(const void *X, long long ldx, const void *Y, long long ldy, float *C, long long ldc, long long R,
                     int N1, int N2, void *workspace, size_t workspace_bytes, epn_stream_t stream);
/* split form of epn_gemm_tn_f32 (see epn_gemm_nt_split_f32).  Wide outputs (N2 >= 512): X, the narrow operand, is split
 * ahead of the GEMM into bf16 planes laid out [plane][R/8][N1][8] in the workspace, Y in registers; narrow ones: both
 * operands in registers.  Workspace size: epn_gemm_tn_workspace_bytes(2, ...); too small -> EPN_EWORKSPACE. */
int epn_gemm_tn_split_f32(const float *X, long long ldx, const float *Y, long long ldy, float *C, long long ldc,
                          long long R, int N1, int N2, void *workspace, size_t workspace_bytes, epn_stream_t stream);
/* Grouped TN (`bf16`: 0 = fp32, 1 = bf16 operands, 2 = fp32 operands in the split form): up to 6 problems in ONE launch (the five weight-gradient GEMMs of a spectral IntraSO3Conv layer, each too
 * small to fill the chip alone); splits are planned so that every workgroup runs about the same number of K steps. */
typedef struct epn_gemm_tn_problem {
    const void *X, *Y;
    float *C;
    long long R, ldx, ldy, ldc;
    int N1, N2;
} epn_gemm_tn_problem;
size_t epn_gemm_tn_grouped_workspace_bytes(int bf16, int nprob, const epn_gemm_tn_problem *probs);
int epn_gemm_tn_grouped(int bf16, int nprob, const epn_gemm_tn_problem *probs, void *workspace, size_t workspace_bytes,
                        epn_stream_t stream);

/* ---- fp32 contractions as THREE fp16 matrix products ("f16x2", round 5; csrc/gemm.h) -------------------------------------
 * Same math as BasicSO3Conv.forward and its autograd transposes (vgtk/vgtk/so3conv/modules.py:48-55), fp32 operands, fp32
 * accumulation, fp32 result.  Each operand is scaled by the power of two that puts its largest magnitude at 2^14 and split
 * into two fp16 pieces x 2^s = h + l (22-23 significant bits for every element within 2^-17 of the tensor's maximum,
 * absolute error <= max|x| 2^-39 below); a product is hh + hl + lh on v_mfma_f32_32x32x16_f16 -- half the matrix
 * instructions of the lossless three-piece bf16 form (epn_gemm_*_split_f32), with a measured error against fp64 at or below
 * that of the fp32 matrix instruction.  The scale comes from a DEVICE scalar holding max|x|: pass the
 * pointer when a producer already knows it (epn_absmax_f32 computes one: memset + one pass), or NULL and the entry point
 * makes that pass itself into its workspace.  Nothing is synchronised with the host; capturable into a HIP graph.
 * `a_amax` / `x_amax` / `y_amax`: arrays of nprob device pointers (entries may be NULL), or NULL.
 * Workspace: epn_gemm_nt_f16x2_workspace_bytes; epn_gemm_tn_workspace_bytes(3, ...) / epn_gemm_tn_grouped_workspace_bytes(3, ...). */
/* The anchor basis change in the fp32 split form + max |out| into the device scalar *amax_out (zeroed by the call): the
 * producer-side maximum of the spectral buffers, so that the two-piece GEMMs that read them need no pass of their own.
 * Arguments as epn_so3_basis_split_f32 / epn_so3_basis_norm_split_f32. */
int epn_so3_basis_amax_split_f32(const float *in, const float *M, const int32_t *blocks, long long pts, int na, int c,
                                 int in_spectral, int out_spectral, float *out, float *amax_out, epn_stream_t stream);
int epn_so3_basis_norm_amax_split_f32(const float *in, const float *M, const int32_t *blocks, long long pts, int na, int c,
                                      int out_spectral, float *out, const float *sums, int groups, long long pts_per_group,
                                      const float *gamma, const float *beta, float eps, float slope, float *amax_out,
                                      epn_stream_t stream);
int epn_absmax_f32(const float *src, long long ld, long long rows, long long cols, float *out, epn_stream_t stream);
size_t epn_gemm_nt_f16x2_workspace_bytes(int nprob, const epn_gemm_nt_problem *probs);
int epn_gemm_nt_f16x2_f32(int nprob, const epn_gemm_nt_problem *probs, const float *const *a_amax, void *workspace,
                          size_t workspace_bytes, epn_stream_t stream);
int epn_gemm_tn_f16x2_f32(const float *X, long long ldx, const float *Y, long long ldy, float *C, long long ldc, long long R,
                          int N1, int N2, const float *x_amax, const float *y_amax, void *workspace, size_t workspace_bytes,
                          epn_stream_t stream);
int epn_gemm_tn_grouped_f16x2(int nprob, const epn_gemm_tn_problem *probs, const float *const *x_amax, const float *const *y_amax,
                              void *workspace, size_t workspace_bytes, epn_stream_t stream);
/* Data gradient of InterSO3Conv with the gradient of the grouped features kept ON CHIP (round 6; csrc/inter_bwd_f2.hip):
 *     grad_feats[b, idx[b,p,n], a, c] (+)= sum_k w[b,p,a,k,n] * sum_o grad_out[col][o] W[o][c*ks + k]
 * -- autograd's transpose of BasicSO3Conv's matmul (vgtk/vgtk/so3conv/modules.py:48-55) chained with the scatter-add that is
 * the backward of inter_zpconv_grouping_naive's gather (vgtk/vgtk/spconv/functional.py:372-390), in ONE kernel: the
 * [cols, cin*ks] gradient of the grouped features (which epn_gemm_nt_f16x2_f32 + epn_inter_ungroup_f32 write to and read back
 * from HBM: 27 GB per classification step) lives in registers.  The contraction over the output channels runs in the two-piece
 * fp16 form (three v_mfma_f32_16x16x32_f16 per block, fp32 accumulate) inside the workgroup of the LDS-pre-reduced scatter.
 * go_amax: device scalar max|grad_out| (required: epn_absmax_f32 computes one).  accumulate != 0: added to what grad_feats_cl
 * holds.  Shapes: ks == 24, 16 <= na <= 64, nn <= 32, cout in {64, 128, 256}, cin % 16 == 0, p2 % 8 == 0 (epn_..._ok). */
int epn_inter_bwd_data_f16x2_ok(const epn_inter_desc *d);
size_t epn_inter_bwd_data_f16x2_workspace_bytes(const epn_inter_desc *d);
int epn_inter_bwd_data_f16x2_f32(const epn_inter_desc *d, const float *grad_out_cl, const float *W, const float *go_amax,
                                 float *grad_feats_cl, int accumulate, void *workspace, size_t workspace_bytes,
                                 epn_stream_t stream);
/* Transpose of the grouping with a whole cloud's gradient rows resident in LDS (round 6; csrc/inter_ungroup_cloud.hip):
 *     grad_feats[b, idx[b,p,n], a, c] = (add[...] +) sum over (p, n) of sum_k w[b,p,a,k,n] * grad_grouped[(b,p,a)][c*ks + k]
 * -- the backward of inter_zpconv_grouping_naive's gather (vgtk/vgtk/spconv/functional.py:372-390), as epn_inter_ungroup_*, with
 * NO global atomics: a workgroup owns every output point of one (cloud, anchor) and with them the destination rows outright,
 * accumulates them in LDS as 64-bit fixed-point integers (integer LDS atomics run at the LDS store rate on gfx950, the
 * floating-point ones 31 x slower) and writes them once.  Consequences: no zero fill of the target, the result is written in the
 * gradient's own type (bf16 entry: bf16 in, bf16 out -- no fp32 scatter target + conversion pass; out_f32 != 0: fp32 out and
 * add, the contract of epn_inter_ungroup_bf16), `add` (same shape and type as
 * grad_feats_cl; may BE grad_feats_cl; or NULL) is folded into the write-out, and the sum does not depend on the order in which
 * waves arrive: bitwise repeatable.
 * Fixed point: unit = max|grad_grouped| * 2^-(43 .. 50) (from the device scalar *dg_amax and the largest multiplicity of the
 * index table; every contribution is rounded ONCE to the unit, the sum is exact, one rounding to the output type).  The index
 * table may be arbitrary: the ball query's cyclic padding is folded into multiplicities, and a row whose remaining slots (all of
 * them if it is not cyclic, one period if it is) still name a point more than once counts with multiplicity nn (those slots are
 * summed one by one, the unit is coarser, down to 2^-39 of the maximum), so that the 64-bit sum of a destination stays below
 * 2^62 units for every table with p2 <= 4096.  dg_amax
 * NULL: the entry takes the maximum itself (one more pass over grad_grouped).  An UNDERSTATED maximum makes contributions leave
 * the representable range: such a workgroup writes NaN to its rows and bumps a sticky device counter
 * (epn_inter_ungroup_cloud_range_count; reset != 0 clears it), as does a non-finite grad_grouped.
 * Shapes (epn_..._ok): the MFMA grouping's (cin % 16 == 0, ks % 4 == 0, ks <= 32, nn <= 64), p2 <= 4096, and p1 small enough
 * for (p1 + 4) * 16 * 8 + 16 bytes of accumulators to fit the 160 KB of a CU's LDS (p1 <= 1275). */
int epn_inter_ungroup_cloud_ok(const epn_inter_desc *d);
size_t epn_inter_ungroup_cloud_workspace_bytes(const epn_inter_desc *d);
int epn_inter_ungroup_cloud_f32(const epn_inter_desc *d, const float *grad_grouped, const float *dg_amax, float *grad_feats_cl,
                                const float *add, void *workspace, size_t workspace_bytes, epn_stream_t stream);
int epn_inter_ungroup_cloud_bf16(const epn_inter_desc *d, const void *grad_grouped, const float *dg_amax, void *grad_feats_cl,
                                 const void *add, int out_f32, void *workspace, size_t workspace_bytes, epn_stream_t stream);
long long epn_inter_ungroup_cloud_range_count(int reset);
/* The scale contract of the two-piece form made loud (round 6).  The power-of-two scale leaves a factor 2-4 below fp16's
 * 65504, so an operand element above 2-4 x the maximum the caller REPORTED becomes inf in the split and the product silently
 * non-finite -- where the fp32 matmul these entry points replace (torch.matmul in vgtk/vgtk/so3conv/modules.py:48-55) would
 * have returned a finite number.  Every two-piece kernel checks its accumulators once per tile in the epilogue; a wave that
 * ends with a non-finite accumulator bumps a sticky per-device counter.  epn_f16x2_overflow_count returns that count for the
 * CURRENT device (reset != 0 also clears it); with finite operands any non-zero value is a violated maximum (a stale or
 * under-reported `*_amax`).  Non-finite operands raise it too (their rows are legitimately non-finite) -- clear the counter
 * after feeding such inputs on purpose.  Synchronous (a 4-byte device read): call it outside timed regions and never during
 * stream capture.  A negative return is a negated hipError_t.  bench.py reports it in its line; tests/conftest.py fails any
 * GPU test that leaves it non-zero. */
long long epn_f16x2_overflow_count(int reset);
/* dst[cols][rows] = src[rows][cols]^T with an optional fp32 <-> bf16 conversion (weights: W^T for the data gradient,
 * bf16 copies of the fp32 master weights); epn_cast converts a flat array. */
int epn_transpose_cast(const void *src, void *dst, int rows, int cols, int src_bf16, int dst_bf16, epn_stream_t stream);
int epn_cast(const void *src, void *dst, size_t n, int src_bf16, int dst_bf16, epn_stream_t stream);
/* dst bf16[n] = bf16(src f32[n] + float(add bf16[n])) in one pass (16-byte aligned pointers): the fp32 scatter target of a
 * bf16 network's InterSO3Conv data gradient converted AND added to the gradient that reached the same tensor through the
 * block's skip branch. */
int epn_cast_add_bf16(const float *src, const void *add, void *dst, size_t n, epn_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * bf16 feature path (BASELINE configs 3-4: "bf16 features / fp32 accumulate"; the reference dispatches float/double only,
 * grouping_cuda_kernel.cu:477,638, so these follow the same interfaces as their _f32 twins with feature tensors stored
 * as bfloat16).  Coordinates, indices, kernel-influence weights w, statistics, affine parameters, weight gradients
 * and every accumulation stay fp32; products inside the GEMMs are bf16 x bf16 -> fp32.
 *   epn_inter_group_bf16   : feats_cl bf16 [b][p1][na][cin] -> grouped bf16 [b*p2*na][cin*ks]   (cin % 16 == 0)
 *   epn_inter_ungroup_bf16 : grad_grouped bf16 -> grad_feats_cl **fp32** (atomic scatter target; convert with epn_cast)
 *   epn_intra_group_bf16   : pure gather of bf16 rows (c % 8 == 0)
 *   epn_so3_basis_bf16, epn_chan_stats_bf16, epn_norm_act_*_bf16: as the _f32 entry points, x / y / dy / dx / residual
 *   in bf16.  The first layer (cin = 1) and PointnetSO3Conv run their fp32 kernels on tensors converted by epn_cast. */
int epn_inter_group_bf16(const epn_inter_desc *d, const void *feats_cl, void *grouped, void *workspace,
                         size_t workspace_bytes, epn_stream_t stream);
int epn_inter_ungroup_bf16(const epn_inter_desc *d, const void *grad_grouped, float *grad_feats_cl, void *workspace,
                           size_t workspace_bytes, epn_stream_t stream);
int epn_intra_group_bf16(const void *feats_cl, const int32_t *intra_idx, void *grouped, int b, int p, int na, int kn,
                         int c, epn_stream_t stream);
int epn_so3_basis_bf16(const void *in, const float *M, const int32_t *blocks, long long pts, int na, int c,
                       int in_spectral, int out_spectral, void *out, epn_stream_t stream);

/* Block glue folded into the basis change ("norm on load", SPConvNets/utils/base_so3conv.py:196-204: InterSO3ConvBlock's
 * norm + leaky_relu feeding IntraSO3Conv): out = basis_change(leaky_relu(norm(in))) with `in` in the plain channels-last
 * layout and sums[g][c] = (sum x, sum x^2) from epn_chan_stats_* (groups = 1: BatchNorm2d, or the number of clouds with
 * pts_per_group points each: InstanceNorm2d; gamma / beta may be NULL).  The normalised tensor is never written. */
int epn_so3_basis_norm_f32(const float *in, const float *M, const int32_t *blocks, long long pts, int na, int c,
                           int out_spectral, float *out, const float *sums, int groups, long long pts_per_group,
                           const float *gamma, const float *beta, float eps, float slope, epn_stream_t stream);
int epn_so3_basis_norm_bf16(const void *in, const float *M, const int32_t *blocks, long long pts, int na, int c,
                            int out_spectral, void *out, const float *sums, int groups, long long pts_per_group,
                            const float *gamma, const float *beta, float eps, float slope, epn_stream_t stream);
/* fp32 in / fp32 out on the bf16 matrix pipe (split form, see epn_gemm_nt_split_f32): M and the input rows are split
 * without loss into three bf16 pieces, six piece products per multiply, fp32 accumulation */
int epn_so3_basis_split_f32(const float *in, const float *M, const int32_t *blocks, long long pts, int na, int c,
                            int in_spectral, int out_spectral, float *out, epn_stream_t stream);
int epn_so3_basis_norm_split_f32(const float *in, const float *M, const int32_t *blocks, long long pts, int na, int c,
                                 int out_spectral, float *out, const float *sums, int groups, long long pts_per_group,
                                 const float *gamma, const float *beta, float eps, float slope, epn_stream_t stream);
/* The twins of epn_so3_basis_norm_* with frozen statistics (see "Frozen statistics" above): stats[c][2] = (mean, var) from
 * epn_bn_frozen_stats_f32, one group.  Replace torch.nn.BatchNorm2d in eval mode + leaky_relu in front of IntraSO3Conv
 * (base_so3conv.py:168-212 / :87-126). */
int epn_so3_basis_norm_frozen_f32(const float *in, const float *M, const int32_t *blocks, long long pts, int na, int c,
                                  int out_spectral, float *out, const float *stats, const float *gamma, const float *beta,
                                  float eps, float slope, epn_stream_t stream);
int epn_so3_basis_norm_frozen_split_f32(const float *in, const float *M, const int32_t *blocks, long long pts, int na, int c,
                                        int out_spectral, float *out, const float *stats, const float *gamma,
                                        const float *beta, float eps, float slope, epn_stream_t stream);
int epn_so3_basis_norm_frozen_bf16(const void *in, const float *M, const int32_t *blocks, long long pts, int na, int c,
                                   int out_spectral, void *out, const float *stats, const float *gamma, const float *beta,
                                   float eps, float slope, epn_stream_t stream);
/* The backward reduction of the block's FIRST norm (InterSO3ConvBlock's norm + leaky_relu in front of IntraSO3Conv,
 * SPConvNets/utils/base_so3conv.py:196-204) taken from the kernel that produces its output gradient: the inverse basis change
 * of the spectral gradient writes dy (plain layout) AND, from its accumulators, per point the partial sums
 *   point_dstats[pt][c][2] = (sum_a d, sum_a d * xhat),   d = dy * leaky'(norm(x)),  xhat = (x - mean) * rstd
 * of the tensor x_cl the forward transform normalised (sums / groups / pts_per_group / gamma / beta / eps / slope as for
 * epn_so3_basis_norm_*).  epn_norm_bwd_finish reduces block partials part[g][block][c][2] to the dsums[g][c][2], dgamma[c],
 * dbeta[c] that epn_norm_act_bwd_apply_* takes (workspace: epn_stats_finish_workspace_bytes(groups, blocks_per_group, c));
 * together they replace epn_norm_act_bwd_reduce_* (one full read of x and dy) for that norm.  Tensors of 2 GiB or more, 2^24
 * points or more, or a point of na * c * 4 >= 2^24 bytes (the shapes the 32-bit-offset kernels do not take): EPN_EINVAL,
 * nothing is written (keep the separate reduction). */
int epn_so3_basis_dstats_f32(const float *in, const float *M, const int32_t *blocks, long long pts, int na, int c, float *out,
                             const float *x_cl, const float *sums, int groups, long long pts_per_group, const float *gamma,
                             const float *beta, float eps, float slope, float *point_dstats, epn_stream_t stream);
int epn_so3_basis_dstats_split_f32(const float *in, const float *M, const int32_t *blocks, long long pts, int na, int c,
                                   float *out, const float *x_cl, const float *sums, int groups, long long pts_per_group,
                                   const float *gamma, const float *beta, float eps, float slope, float *point_dstats,
                                   epn_stream_t stream);
int epn_so3_basis_dstats_bf16(const void *in, const float *M, const int32_t *blocks, long long pts, int na, int c, void *out,
                              const void *x_cl, const float *sums, int groups, long long pts_per_group, const float *gamma,
                              const float *beta, float eps, float slope, float *point_dstats, epn_stream_t stream);
int epn_norm_bwd_finish(const float *partials, int groups, long long blocks_per_group, int c, const float *gamma,
                        float *dsums, float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes,
                        epn_stream_t stream);
int epn_chan_stats_bf16(const void *x_cl, int groups, long long rows, int c, float *sums, void *workspace,
                        size_t workspace_bytes, epn_stream_t stream);
int epn_norm_act_fwd_bf16(const void *x_cl, int groups, long long rows, int c, const float *sums, const float *gamma,
                          const float *beta, const void *residual_cl, float eps, float slope, void *y_cl,
                          epn_stream_t stream);
int epn_norm_act_bwd_reduce_bf16(const void *x_cl, const void *dy_cl, int groups, long long rows, int c,
                                 const float *sums, const float *gamma, const float *beta, float eps, float slope,
                                 float *dsums, float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes,
                                 epn_stream_t stream);
int epn_norm_act_bwd_apply_bf16(const void *x_cl, const void *dy_cl, int groups, long long rows, int c,
                                const float *sums, const float *dsums, const float *gamma, const float *beta, float eps,
                                float slope, void *dx_cl, epn_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * Deterministic (atomic-free) data gradient of the grouping -- the transpose of epn_inter_group_* without the fp32 atomic
 * scatter of epn_inter_ungroup_* (reference: torch autograd through gather + einsum, whose index_add is itself
 * non-deterministic on CUDA; SURVEY a17 asked for an atomic-free form):
 *   1. epn_inter_inverse_list: ball_idx i32[b][p2][nn] -> CSR per cloud, offsets i32[b][p1+1], entries i32[b][p2*nn]
 *      (entry = p*nn + n with ball_idx[b][p][n] == q, in increasing order) -- once per geometry;
 *   2. epn_inter_ungroup_det_*: per-slot contributions slab[b][p][n][a][c] = sum_k w * grad_grouped (plain stores;
 *      slab has the element type of grad_grouped, b*p2*nn*na*cin elements), then grad_feats_cl[b][q][a][c] = the sum
 *      over q's list in list order (fp32 accumulation; fully overwritten; f32 -> float, bf16 -> bf16 output).
 *      When slab_bytes leaves room for b*p2*nn more bytes behind the (256-byte rounded) slab and the output points
 *      divide into the scatter's workgroups, the contributions are pre-reduced: a workgroup of 8-16 spatially adjacent
 *      output points sums the slots of each distinct destination in LDS (ascending slot order) and stores ONE slab row
 *      per destination, marked in those bytes; step 2 adds only the marked rows (a third of the slab traffic).
 * Bitwise repeatable.  Requires cin % 16 == 0 and na >= 16 (the MFMA grouping kernels). */
int epn_inter_inverse_list(const int32_t *ball_idx, int b, int p1, int p2, int nn, int32_t *offsets, int32_t *entries,
                           epn_stream_t stream);
int epn_inter_ungroup_det_f32(const epn_inter_desc *d, const float *grad_grouped, float *grad_feats_cl,
                              const int32_t *offsets, const int32_t *entries, void *slab, size_t slab_bytes,
                              void *workspace, size_t workspace_bytes, epn_stream_t stream);
int epn_inter_ungroup_det_bf16(const epn_inter_desc *d, const void *grad_grouped, void *grad_feats_cl,
                               const int32_t *offsets, const int32_t *entries, void *slab, size_t slab_bytes,
                               void *workspace, size_t workspace_bytes, epn_stream_t stream);

/* Strided skip connection of SeparableSO3ConvBlock: replaces zptk.functional.batched_index_select(skip_feature, 2,
 * sample_idx) (SPConvNets/utils/base_so3conv.py:206-207; vgtk/vgtk/spconv/functional.py:361-369: torch.gather with a
 * broadcast index) on channels-last data, where it is a gather of whole [a][c] rows, and its autograd backward.
 *   src [b][p1][row_bytes], idx i32[b][p2] -> dst [b][p2][row_bytes]            (row_bytes % 16 == 0, any element type)
 *   epn_scatter_rows: grad_src [b][p1][row_bytes] = 0, then row idx[b][p] <- grad_dst[b][p] (indices distinct per cloud,
 *   as FPS indices are: plain stores, deterministic)
 * An index outside [0, p1) is skipped by all three entries: epn_gather_rows does NOT write that destination row (it keeps
 * whatever it held), epn_scatter_rows / epn_scatter_rows_add neither store nor add that gradient row. */
int epn_gather_rows(const void *src, const int32_t *idx, void *dst, int b, int p1, int p2, long long row_bytes,
                    epn_stream_t stream);
int epn_scatter_rows(const void *grad_dst, const int32_t *idx, void *grad_src, int b, int p1, int p2, long long row_bytes,
                     epn_stream_t stream);
/* epn_scatter_rows that ACCUMULATES (atomic-free and deterministic: the first occurrence of an index sums all of its
 * rows in fp32, ascending row order; p2 <= 8192): repeated indices -- FPS repeats index 0 for clouds with fewer live
 * points than samples -- receive the sum of their rows, like the backward of torch.gather / batched_index_select
 * (vgtk/vgtk/spconv/functional.py:28-40).  Elements fp32 (bf16 = 0) or bf16 (bf16 = 1). */
int epn_scatter_rows_add(const void *grad_dst, const int32_t *idx, void *grad_src, int b, int p1, int p2,
                         long long row_bytes, int bf16, epn_stream_t stream);

/* 1x1 convolution of a SINGLE input channel (the skip branch of every model's first block, whose input is the
 * occupancy feature: nn.Conv2d(1, cout, 1), SPConvNets/utils/base_so3conv.py:186): y[row][c] = x[row] * w[c], rows =
 * b*p*a of the channels-last tensor, cout % 4 == 0; and its weight gradient grad_w[c] = sum_row x[row] * grad_y[row][c]
 * (zero-fills grad_w first; 256 % (cout/4) == 0).  epn_conv1x1_c1_bwd_weight_f32 adds its per-block partials with fp32
 * atomics, in an order that varies from call to call; epn_conv1x1_c1_bwd_weight_ws_f32 stores them to `workspace` (16-byte
 * aligned, at least EPN_CONV1X1_C1_WS_BYTES(cout) bytes; EPN_EWORKSPACE below what the call needs) and sums them in a fixed
 * order: bitwise repeatable.  Behind an instance norm the gradient is a near-cancelling sum, where the atomics' order moves
 * it by tens of percent. */
#define EPN_CONV1X1_C1_WS_BYTES(cout) ((size_t)1024 * (size_t)(cout) * sizeof(float))
int epn_conv1x1_c1_f32(const float *x, const float *w, float *y, long long rows, int cout, epn_stream_t stream);
int epn_conv1x1_c1_bwd_weight_f32(const float *x, const float *grad_y, float *grad_w, long long rows, int cout,
                                  epn_stream_t stream);
int epn_conv1x1_c1_bwd_weight_ws_f32(const float *x, const float *grad_y, float *grad_w, long long rows, int cout,
                                     void *workspace, size_t workspace_bytes, epn_stream_t stream);

/* Attention pooling over the anchors in the 3DMatch head: replaces `attn = F.softmax(attn, dim=3)` and
 * `x_out = (x.feats * attn).sum(-1, keepdim=True)` of InvOutBlockMVD.forward (SPConvNets/utils/base_so3conv.py:603-606)
 * and their autograd backward, on channels-last rows [row = (b, p)][a][c] (na <= 64):
 *   fwd: attn[row][a][c] = softmax over a of logits[row][a][c];  pooled[row][c] = sum_a feats[row][a][c] * attn[row][a][c]
 *   bwd: g = grad_pooled * feats (+ grad_attn);  grad_logits = attn * (g - sum_a attn g);  grad_feats = grad_pooled * attn
 *        grad_pooled or grad_attn_cl may be NULL (not both: EPN_ENULL), grad_feats_cl may be NULL (not wanted). */
int epn_anchor_softmax_pool_fwd_f32(const float *feats_cl, const float *logits_cl, float *attn_cl, float *pooled,
                                    long long rows, int na, int c, epn_stream_t stream);
int epn_anchor_softmax_pool_bwd_f32(const float *feats_cl, const float *attn_cl, const float *grad_pooled,
                                    const float *grad_attn_cl, float *grad_feats_cl, float *grad_logits_cl,
                                    long long rows, int na, int c, epn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EPN_SO3CONV_H */
