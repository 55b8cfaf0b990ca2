/*
 * mipsf_track_color.h -- mipsf_track_register (mipsf_track.h) with a photometric term: the live frame's colour against the colour
 * image of the same ray cast, so that the registration holds where the depth alone leaves the pose free -- along a wall, along the
 * edge two walls share.  DESIGN.md 4.23; mipsfusion_amd/tsdf.py.  The declarations of mipsf_track.h are untouched; this file adds
 * one entry point and one `which` of mipsf_track_workspace_bytes.
 *
 * The conventions are those of mipsf_track.h: int return code, message through mipsf_last_error(), one argument block with
 * `struct_size` first, DEVICE pointers, everything enqueued on `stream`, no allocation and no synchronisation, the caller's
 * workspace, no floating-point atomic, the same bytes from the same call.  Every floating-point operation named below is one IEEE
 * float64 operation rounded on its own (no contraction, no reciprocal), fp32 inputs widened first, and only + - * /, sqrt and floor
 * occur, so the float64 restatement on the host (tests/track_color_cpu.py) gives the same words.
 */
#ifndef MIPSF_TRACK_COLOR_H
#define MIPSF_TRACK_COLOR_H

#include "mipsf_track.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MIPSF_TRACK_COLOR_RESULT_DOUBLES 22u     /* MIPSF_TRACK_RESULT_DOUBLES, photometric rows, their rmse                     */

/* mipsf_track_workspace_bytes(which, a, b, c) */
#define MIPSF_TRACK_WS_REGISTER_COLOR 3          /* a, b = H, W                                                                  */

/* mipsf_track_register_color: model_depth, model_normals and model_color fp32 [H,W,3] are one view of ONE mipsf_track_raycast
 * (depth, normals, color_out), cast from pose_ref; live and live_color fp32 [H,W,3] are the frame.  Everything mipsf_track_register
 * says about its arguments, T, the evaluations and the outputs holds here.
 *
 * One evaluation.  A live pixel (row, col) makes a geometric pair exactly when it does in mipsf_track_register, with the same p,
 * cam, z, u, v, row2, col2, dm, nrm, d2 and r.  Such a pair also gives a PHOTOMETRIC ROW when all of this holds:
 *   c0 = floor(u);  r0 = floor(v);  0 <= c0 && c0 + 1 < W && 0 <= r0 && r0 + 1 < H           (the 2 x 2 patch around (v, u))
 *   the four model_depth words at (r0, c0), (r0, c0+1), (r0+1, c0), (r0+1, c0+1), widened, are each > 0 and < inf
 *   intensity of a colour triple (r, g, b):  I = (((double)r + (double)g) + (double)b) / 3.0
 *        I00, I01, I10, I11 of model_color at those four pixels in that order, Il of live_color[row][col]; nothing is stored
 *   fu = u - c0;  fv = v - r0
 *   Im = (I00*(1 - fu) + I01*fu)*(1 - fv) + (I10*(1 - fu) + I11*fu)*fv
 *   Iu = (I01 - I00)*(1 - fv) + (I11 - I10)*fv
 *   Iv = (I10 - I00)*(1 - fu) + (I11 - I01)*fu          (the bilinear patch and its own derivatives: no gradient image, no pass)
 *   rI = Im - Il;  fabs(rI) <= max_color_diff && fabs(rI) < inf
 * A NaN anywhere makes the last line false, and so does an infinite colour word (it gives an infinite or NaN rI); either drops the
 * row, never the pair.  A row has only finite terms.  Its direction in the reference camera's frame and in the world:
 *   g_cam = ( Iu*(fx/z),  -(Iv*(fy/z)),  Iu*(fx*(cam.x/(z*z))) - Iv*(fy*(cam.y/(z*z))) )
 *   g[r]  = (R_ref[r][0]*g_cam.x + R_ref[r][1]*g_cam.y) + R_ref[r][2]*g_cam.z
 * and its Jacobian is Jc = (p x g, g), the form of J = (p x nrm, nrm).
 *
 * Sums.  Columns 0 .. 26 are those of mipsf_track_register (the upper triangle row by row, then J^T r): with geo_k the lane's share
 * there (J[a]*J[b], J[a]*r) and col_k the same products of Jc and rI (Jc[a]*Jc[b], Jc[a]*rI), the lane's share here is
 * geo_k + color_weight*col_k for a pair with a photometric row and geo_k itself for a pair without.  Columns 27, 28, 29: pairs, sum
 * of d2, usable pixels, as there.  Column 30: photometric rows.  Column 31: the sum of rI*rI.  Lane -> wave -> block of 256 pixels
 * in row-major order -> in block order, as there.
 *
 * The judgement, the Cholesky, the update and the `done` word are those of mipsf_track_register, with color_rmse =
 * sqrt(column 31 / column 30) (0 without rows) and one change to the stop: the relative stop also needs
 * fabs(prev_color_rmse - color_rmse) < relative_color_rmse.  (On a lone wall fitness and inlier rmse stand still while the colour
 * moves the pose along the plane.)  With color_weight = 0 and relative_color_rmse = +inf the first 20 result doubles and pose_out
 * are mipsf_track_register's, bit for bit, as long as the colour words are finite.  max_iteration + 1 evaluations are enqueued.
 *
 * result: MIPSF_TRACK_COLOR_RESULT_DOUBLES doubles -- the 20 of mipsf_track_register, then the photometric rows of the judged
 * evaluation and color_rmse.  pose_out, partner: as there.  color_partner (optional) int32 [H,W]: 1 where the live pixel gave a
 * photometric row in the last evaluation, else 0.
 * Refused on the host: everything mipsf_track_register refuses; color_weight negative, infinite or NaN; max_color_diff negative
 * or NaN (+inf keeps every finite row); relative_color_rmse NaN; a null model_color or live_color. */
typedef struct mipsf_track_register_color_args {
    uint32_t struct_size;
    uint32_t H, W;
    uint32_t max_iteration;
    double fx, fy, cx, cy, depth_max, max_dist, relative_fitness, relative_rmse;
    double color_weight, max_color_diff, relative_color_rmse;
    const float* model_depth;           /* [H,W]                                                                               */
    const float* model_normals;         /* [H,W,3]                                                                             */
    const float* model_color;           /* [H,W,3]                                                                             */
    const float* pose_ref;              /* [4,4]                                                                               */
    const float* live;                  /* [H,W]                                                                               */
    const float* live_color;            /* [H,W,3]                                                                             */
    const float* pose_init;             /* [4,4]                                                                               */
    double* result;                     /* [MIPSF_TRACK_COLOR_RESULT_DOUBLES]                                                  */
    float* pose_out;                    /* [4,4]                                                                               */
    int32_t* partner;                   /* [H,W] or null                                                                       */
    int32_t* color_partner;             /* [H,W] or null                                                                       */
    void* workspace;                    /* mipsf_track_workspace_bytes(MIPSF_TRACK_WS_REGISTER_COLOR, H, W, 0)                  */
} mipsf_track_register_color_args;

int mipsf_track_register_color(const mipsf_track_register_color_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIPSF_TRACK_COLOR_H */
