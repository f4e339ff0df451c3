// error.cpp -- per-thread error string + ABI version of libancsh_hip.so.
#include "common.h"

namespace ancsh {
static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
}  // namespace ancsh

extern "C" int ancsh_abi_version(void) { return 14; }   // added since without a new number (callers detect them by their symbols): ancsh_depth_unproject_stream, ancsh_depth_label_images (the depth front end and its label / NOCS images), ancsh_depth_annotated_images (predicted and true part / NOCS images of annotated frames), ancsh_pose_fit_rec* (both stages of the pose fit in one call); 14: + ancsh_ransac_joint_rec_kind, ancsh_ransac_joint_rec_dseed_kind, ancsh_ransac_joint_rec_dkey_kind (a joint kind per stage-B problem: the prismatic objective); 13: + ancsh_pose_joint_direction_pred, ancsh_pose_poison_records_pred, ancsh_input_sample_stream_xyz, ancsh_input_sample_stream_xyz_keyed (the predicted joint association and xyz-only raw rows); 12: + ancsh_raw_point_labels (per-raw-point labels and head values of a streamed batch); 11: + ancsh_articulation_rec (the streamed articulation block: part boxes and camera-space joints); 10: + ancsh_input_sample_stream_keyed, ancsh_ransac_single_rec_dkey, ancsh_ransac_joint_rec_dkey (the ancsh_stream_key block: a global cloud base next to the device key, for sharded streams); 9: + the F16x2 range guard (ancsh_*_f16x2*_guarded); 8: + ancsh_input_sample_stream, ancsh_ransac_single_rec_dseed, ancsh_ransac_joint_rec_dseed (device-memory sizes and seeds for the captured streaming step); 7: ancsh_hbm_copy (a bench yardstick, not an operator) moved out of the library into tools/microbench; 6: + the split-16 experiment's grouped / tail / F16x2 entry points (ancsh_*_bf16x3_grouped, ancsh_mlp_chain_grouped_fp_bf16x3, ancsh_*_f16x2*), ancsh_pose_poison_records; tie_stats[1] of ancsh_ransac_single_rec redefined (sign = degenerate winner); 5: + the mid-section chains (ancsh_sa3_chain_grouped, ancsh_fp_single_source_init, ancsh_fp1_chain_grouped, ancsh_fp2_chain_grouped), ancsh_mlp_chain_grouped_fp, ancsh_ransac_single_rec / ancsh_ransac_joint_rec, ancsh_last_ball_query_schedule; 4: + ancsh_joint_params, ancsh_part_extents, ancsh_query_ball_group_xyz_multi; LM_AUTO = THROUGHPUT (3: grouped launches, ancsh_ransac_single_ex, ancsh_three_nn_weights; additions only)
extern "C" const char *ancsh_last_error(void) { return ancsh::g_err; }
