// session_edit.hip -- what an edit of the session's click list (undo, redo, remove, restore) rebuilds on the device (gfx950):
// the relabelled ground truth of the list and the renumbering of the last inference's labels.
//
// The reference has no counterpart: its GUI leaves "unselect point" as a TODO (interactive_tool/gui.py:283-287) and relabels
// the ground truth click by click (gui.py:318-319, one torch boolean-index pass per new object), which cannot be rolled
// back.  THE RULE (ours, stated in include/agile3d_hip.h at a3d_session_edit):
//   relabel   new_labels[i] = the largest k in 1..n_objects with instances[k - 1] == labels_ori[i], else 0
//   remap     labels[i] = lut[labels[i]] in place; a value outside 0..255 writes 0 and raises the flag
// Both halves are streaming grid-stride passes over 4-byte rows, 8 bytes of traffic per row, ONE launch for the two.  The
// two tables (at most 255 instance ids, the 256-byte lut) are staged in LDS once per workgroup; the relabel walks its table
// from the top and leaves at the first match -- every lane reads the same LDS address, a broadcast, as the marker and cube
// walks of session.hip do.  No workspace, no atomic on a result (only the flag), nothing depends on the order of workgroups.
#include "common.h"

namespace a3d {

constexpr int kEditBlock = 256;
constexpr int kEditMaxBlocks = 1024;          // 4 workgroups per CU; longer inputs take further passes of the grid

__global__ __launch_bounds__(kEditBlock) void k_session_edit(const a3d_session_edit_args a) {
  __shared__ int32_t inst[256];
  __shared__ int32_t lut[256];
  const bool relabel = a.new_labels_dev != nullptr && a.n_full > 0;
  const bool remap = a.labels_dev != nullptr && a.n_labels > 0;
  if (relabel && (int)threadIdx.x < a.n_objects) inst[threadIdx.x] = a.instances_dev[threadIdx.x];
  if (remap) lut[threadIdx.x] = a.lut[threadIdx.x];      // (kEditBlock == 256: one entry per thread)
  __syncthreads();
  const long long first = (long long)blockIdx.x * kEditBlock + threadIdx.x;
  const long long stride = (long long)gridDim.x * kEditBlock;
  if (relabel) {
    for (long long i = first; i < a.n_full; i += stride) {
      const int32_t v = a.labels_ori_dev[i];
      int32_t k = a.n_objects;
      while (k > 0 && inst[k - 1] != v) --k;            // the highest object that claims the instance; 0 = none
      a.new_labels_dev[i] = k;
    }
  }
  if (remap) {
    for (long long i = first; i < a.n_labels; i += stride) {
      const int32_t v = a.labels_dev[i];
      int32_t w = 0;
      if (v < 0 || v > 255)
        atomicOr(a.err_dev, 1);                         // reported through the flag, as a3d_session_paint does
      else
        w = lut[v];
      a.labels_dev[i] = w;
    }
  }
}

}  // namespace a3d

using namespace a3d;

extern "C" int a3d_session_edit(const a3d_session_edit_args* args, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!args) {
    set_error("a3d_session_edit: no arguments");
    return A3D_ERR_INVALID;
  }
  const a3d_session_edit_args& a = *args;
  const bool bad_relabel = a.n_full < 0 || a.n_objects < 0 || a.n_objects > 255 ||
                           (a.n_full > 0 && (!a.new_labels_dev || !a.labels_ori_dev || (a.n_objects > 0 && !a.instances_dev)));
  const bool bad_remap = a.n_labels < 0 || (a.n_labels > 0 && (!a.labels_dev || !a.err_dev));
  if (bad_relabel || bad_remap) {
    set_error("a3d_session_edit: bad arguments (n_full=%lld n_objects=%d n_labels=%lld)", (long long)a.n_full, a.n_objects,
              (long long)a.n_labels);
    return A3D_ERR_INVALID;
  }
  if (a.err_dev) A3D_HIP_CHECK(hipMemsetAsync(a.err_dev, 0, sizeof(int32_t), st));
  const long long n = a.n_full > a.n_labels ? a.n_full : a.n_labels;
  if (n == 0) return A3D_OK;
  const long long want = (n + kEditBlock - 1) / kEditBlock;
  k_session_edit<<<(unsigned)(want < kEditMaxBlocks ? want : kEditMaxBlocks), kEditBlock, 0, st>>>(a);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}
