// HIP kernel (gfx950) of the contact update -- the feet in the world, the terrain under them, the next tick's support flags --
// and its entries of the C-ABI (include/qlamd_contact_detection.h, which qlamd.h includes).  The arithmetic is
// csrc/contact_update_core.hpp's.
#include "contact_update_body.hpp"

using namespace qlamd;
using namespace qlamd::rt;

namespace {

// The body without the anchors (csrc/contact_update_body.hpp).
__global__ __launch_bounds__(kUpdateBlock) void contact_update_kernel(const DeviceParams *Pp, const UpdateIn s, const UpdateGrid G,
                                                                      const ContactRule rule, int64_t B, const UpdateOut o) {
  __shared__ double tab[4 * kTabPerLeg];
  contact_update_body<false>(tab, Pp, s, G, rule, 0u, B, o);
}

} // namespace

extern "C" {

void qlamd_contact_update_default(qlamd_contact_update *u) {
  if (!u) return;
  memset(u, 0, sizeof(*u)); // (the padding too)
  u->plane = nullptr; u->heightfield = nullptr; u->contact_report = nullptr;
  u->release_mask = QLAMD_CONTACT_PULLS;
  u->touchdown_distance = 0.0; u->approach_speed = 0.0; u->liftoff_distance = 0.0; u->sensor_distance = 0.0;
  u->support_next = nullptr; u->contact_sensor = nullptr; u->events = nullptr;
  u->gap = nullptr; u->surface_normal = nullptr; u->foot_position = nullptr; u->foot_velocity = nullptr;
}

int qlamd_wholebody_contact_update_batch(qlamd_context *ctx, const qlamd_wholebody_batch *in, const double *base_position,
                                         const qlamd_contact_update *update, int64_t batch, int32_t *status, int memory,
                                         void *stream) {
  if (const int rc = contact_update_check(ctx, in, base_position, update, batch, status, memory)) return rc;
  if (batch == 0) return QLAMD_OK;
  if (hipSetDevice(ctx->device) != hipSuccess) return QLAMD_ERR_HIP;
  hipStream_t st = (hipStream_t)stream;
  QL_ENTER(ctx, st);
  UpdateCall k = contact_update_call(in, base_position, update, status, nullptr);
  Staged sg(memory == QLAMD_MEM_HOST);
  contact_update_stage(sg, k, update->heightfield, (size_t)batch, ctx->params.keep_on_failure != 0);
  if (const int rc = sg.upload(ctx, st)) return rc;
  const unsigned grid = (unsigned)((4 * batch + kUpdateBlock - 1) / kUpdateBlock);
  hipLaunchKernelGGL(contact_update_kernel, dim3(grid), dim3(kUpdateBlock), 0, st, ctx->d_params, k.s, k.G, k.rule, batch,
                     static_cast<const UpdateOut &>(k.o));
  if (hipGetLastError() != hipSuccess) return QLAMD_ERR_HIP;
  return sg.finish(st);
}

} // extern "C"
