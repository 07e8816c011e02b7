// The contact update, once: the kernel arguments, the body of contact_update_kernel (contact_update_kernel.hip) and of
// anchored_contact_update_kernel (contact_anchor_kernel.hip), and what their two entries check and stage.  kAnchored adds the
// anchor rule, the re-anchored event bit and the three anchor stores; nothing else differs.  The arithmetic is
// csrc/contact_update_core.hpp's.
#pragma once
#include <type_traits>
#include "contact_update_core.hpp"
#include "context.hpp"

namespace qlamd {
namespace rt {

// (no __restrict__ anywhere: support_next may be the array the current flags are read from)
struct UpdateIn {
  const double *q, *qd, *quat, *linvel, *angvel, *pos;
  const uint8_t *stance;   // or NULL: no foot is flagged
  const uint8_t *report;   // or NULL
  const double *plane;     // or NULL
  const double *heights;   // or NULL; with plane NULL as well: the ground z = 0
};
struct UpdateGrid { double ox, oy, inv_res; int nx, ny; };
struct UpdateOut {
  uint8_t *next, *sensor, *events;    // each or NULL
  double *gap, *normal, *fpos, *fvel; // each or NULL
  int32_t *status;
};
struct AnchoredUpdateOut : UpdateOut {
  double *anchor;                     // never read
};

constexpr int kUpdateBlock = 256; // 64 robots per block: the model table is staged once for 256 lanes, two loads each
constexpr unsigned kEventReanchored = 8;

// the bytes of a quad's four lanes, each in its own byte of the word, OR-ed into one word that all four lanes hold
__device__ __forceinline__ uint32_t quad_or(uint32_t x) {
  x |= (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0xB1, 0xF, 0xF, true); // quad_perm [1, 0, 3, 2]
  x |= (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x4E, 0xF, 0xF, true); // quad_perm [2, 3, 0, 1]
  return x;
}

// One lane per (robot, leg), 16 robots per wavefront: the four legs of a robot are independent, only the status is the robot's
// (a quad-wide vote).  Everything is loaded before the first store; the anchors are only written.  A streaming kernel: 336 bytes
// read per robot, and 336 (432 with the anchors) written with every array given.  tab: 4 * kTabPerLeg doubles of LDS.
template <bool kAnchored>
__device__ __forceinline__ void contact_update_body(double *tab, const DeviceParams *Pp, const UpdateIn &s, const UpdateGrid &G,
                                                    const ContactRule &rule, unsigned reanchor, int64_t B,
                                                    const std::conditional_t<kAnchored, AnchoredUpdateOut, UpdateOut> &o) {
  const DeviceParams &P = *Pp;
  const int second = (int)threadIdx.x + kUpdateBlock < 4 * kTabPerLeg ? (int)threadIdx.x + kUpdateBlock : 4 * kTabPerLeg - 1;
  const double tab0 = P.legtab[threadIdx.x], tab1 = P.legtab[second];
  const int64_t t0 = (int64_t)blockIdx.x * kUpdateBlock + threadIdx.x;
  const bool live = t0 < 4 * B; // a quad is live or dead as a whole
  const int64_t t = live ? t0 : 4 * B - 1;
  const int64_t i = t >> 2;
  const int leg = (int)(t & 3);
  double q[3], qd[3], quat[4], linvel[3], angvel[3], pos[3];
  load3(s.q, t, q); load3(s.qd, t, qd);
  {
    const double2 *a2 = reinterpret_cast<const double2 *>(s.quat + 4 * i);
    double2 v = a2[0]; quat[0] = v.x; quat[1] = v.y;
    v = a2[1]; quat[2] = v.x; quat[3] = v.y;
  }
  load3(s.linvel, i, linvel); load3(s.angvel, i, angvel); load3(s.pos, i, pos);
  const uint32_t sw = s.stance ? *reinterpret_cast<const uint32_t *>(s.stance + 4 * i) : 0u;
  const uint32_t rw = s.report ? *reinterpret_cast<const uint32_t *>(s.report + 4 * i) : 0u;
  double pl[4] = {0.0, 0.0, 1.0, 0.0};
  if (s.plane) {
    const double2 *a2 = reinterpret_cast<const double2 *>(s.plane + 4 * i);
    double2 v = a2[0]; pl[0] = v.x; pl[1] = v.y;
    v = a2[1]; pl[2] = v.x; pl[3] = v.y;
  }
  tab[threadIdx.x] = tab0;
  if ((int)threadIdx.x + kUpdateBlock < 4 * kTabPerLeg) tab[threadIdx.x + kUpdateBlock] = tab1;
  __syncthreads();

  double Rm[9], p[3], u[3], n[3], gap;
  quat_to_matrix(quat, Rm);
  cu_foot_world(LdsTab{tab + kTabPerLeg * leg}, q, qd, Rm, pos, linvel, angvel, p, u);
  bool good = cu_finite3(q) && cu_finite3(qd) && cu_finite3(linvel) && cu_finite3(angvel) && cu_finite3(pos) && cu_finite3(p) &&
              cu_finite3(u) && cu_finite(quat[0]) && cu_finite(quat[1]) && cu_finite(quat[2]) && cu_finite(quat[3]);
  if (s.heights) { // (the same on every lane: a kernel argument)
    int ci, cj;
    double alpha, beta;
    cu_cell(p[0], G.ox, G.inv_res, G.nx, ci, alpha);
    cu_cell(p[1], G.oy, G.inv_res, G.ny, cj, beta);
    const double *h = s.heights + ((int64_t)cj * G.nx + ci); // cell (ci, cj) and its three neighbours: inside [ny][nx]
    const double h00 = h[0], h10 = h[1], h01 = h[G.nx], h11 = h[G.nx + 1];
    cu_patch(h00, h10, h01, h11, alpha, beta, G.inv_res, p[2], n, gap);
    good = good && cu_finite(h00) && cu_finite(h10) && cu_finite(h01) && cu_finite(h11);
  } else {
    good = cu_plane(pl, p, n, gap) && good && cu_finite(pl[0]) && cu_finite(pl[1]) && cu_finite(pl[2]) && cu_finite(pl[3]);
  }
  good = good && cu_finite(gap) && cu_finite3(n);
  const bool ok = quad_or(good ? 0u : 1u) == 0u;

  bool next, sensor;
  unsigned events;
  const bool cur = ((sw >> (8 * leg)) & 0xFFu) != 0u;
  const unsigned report = (rw >> (8 * leg)) & 0xFFu; // (0 without a report: no leg is re-anchored then)
  cu_flags(rule, cur, report, gap, dot3(n, u), next, events, sensor);
  bool kept = false;
  if constexpr (kAnchored) {
    // the anchor rule: a foot that stays held keeps its anchor unless the report says it slid
    const bool moved = next && cur && (report & reanchor) != 0u;
    kept = next && cur && !moved;
    events |= moved ? kEventReanchored : 0u;
  }
  const uint32_t next_w = quad_or((next ? 1u : 0u) << (8 * leg)), sensor_w = quad_or((sensor ? 1u : 0u) << (8 * leg)),
                 events_w = quad_or(events << (8 * leg));

  // ---- outputs.  A failed robot: its current flags and zeros, or (QLAMD_ON_FAILURE_KEEP) nothing but its status; its anchors
  // stay as they are either way
  if (!live) return;
  if (leg == 0) o.status[i] = ok ? kStatusOk : kStatusNotPd;
  if (!ok && P.keep_on_failure) return;
  if (leg == 0) {
    if (o.next) *reinterpret_cast<uint32_t *>(o.next + 4 * i) = ok ? next_w : sw;
    if (o.sensor) *reinterpret_cast<uint32_t *>(o.sensor + 4 * i) = ok ? sensor_w : 0u;
    if (o.events) *reinterpret_cast<uint32_t *>(o.events + 4 * i) = ok ? events_w : 0u;
  }
  if (o.gap) o.gap[t] = ok ? gap : 0.0;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    if (o.normal) o.normal[3 * t + a] = ok ? n[a] : 0.0;
    if (o.fpos) o.fpos[3 * t + a] = ok ? p[a] : 0.0;
    if (o.fvel) o.fvel[3 * t + a] = ok ? u[a] : 0.0;
  }
  if constexpr (kAnchored) {
    if (ok && !kept) {
      // a foot held from now on: its projection on the terrain's tangent plane; a free foot: where it is
#pragma unroll
      for (int a = 0; a < 3; a++) o.anchor[3 * t + a] = next ? p[a] - gap * n[a] : p[a];
    }
  }
}

// ---- the host side of the two entries

// What both entries refuse.  (The anchored entry refuses a NULL anchor array as well, at the entry.)
inline int contact_update_check(const qlamd_context *ctx, const qlamd_wholebody_batch *in, const double *base_position,
                                const qlamd_contact_update *update, int64_t batch, const int32_t *status, int memory) {
  if (!ctx || !in || !base_position || !update || !status || batch < 0) return QLAMD_ERR_INVALID_ARGUMENT;
  if (!in->joint_position || !in->joint_velocity || !in->base_orientation || !in->base_linear_velocity ||
      !in->base_angular_velocity)
    return QLAMD_ERR_INVALID_ARGUMENT;
  const qlamd_heightfield *hf = update->heightfield;
  if (update->plane && hf) return QLAMD_ERR_INVALID_ARGUMENT;
  if (hf && (hf->nx < 2 || hf->ny < 2 || !(hf->resolution > 0.0) || !cu_finite(hf->resolution) || !hf->heights))
    return QLAMD_ERR_INVALID_ARGUMENT;
  if (!cu_finite(update->touchdown_distance) || !cu_finite(update->approach_speed) || !cu_finite(update->liftoff_distance) ||
      !cu_finite(update->sensor_distance) || update->liftoff_distance < update->touchdown_distance)
    return QLAMD_ERR_INVALID_ARGUMENT;
  if (memory != QLAMD_MEM_DEVICE && memory != QLAMD_MEM_HOST) return QLAMD_ERR_INVALID_ARGUMENT;
  return QLAMD_OK;
}

// The kernel arguments of one call; anchor: NULL for the entry without anchors.
struct UpdateCall {
  UpdateIn s;
  UpdateGrid G;
  ContactRule rule;
  AnchoredUpdateOut o;
};
inline UpdateCall contact_update_call(const qlamd_wholebody_batch *in, const double *base_position, const qlamd_contact_update *update,
                                      int32_t *status, double *anchor) {
  const qlamd_heightfield *hf = update->heightfield;
  UpdateCall k{};
  k.s = UpdateIn{in->joint_position, in->joint_velocity, in->base_orientation, in->base_linear_velocity, in->base_angular_velocity,
                 base_position, in->support_leg, update->contact_report, update->plane, hf ? hf->heights : nullptr};
  k.G = hf ? UpdateGrid{hf->origin_x, hf->origin_y, 1.0 / hf->resolution, hf->nx, hf->ny} : UpdateGrid{0.0, 0.0, 1.0, 2, 2};
  k.rule = ContactRule{update->touchdown_distance, update->approach_speed, update->liftoff_distance, update->sensor_distance,
                       update->release_mask};
  k.o = AnchoredUpdateOut{{update->support_next, update->contact_sensor, update->events, update->gap, update->surface_normal,
                           update->foot_position, update->foot_velocity, status}, anchor};
  return k;
}

// Binds every array of the call (a NULL one stages nothing).  keep: entries the kernel leaves alone come back as they went up;
// kept anchors always do.
inline void contact_update_stage(Staged &sg, UpdateCall &k, const qlamd_heightfield *hf, size_t B, bool keep) {
  UpdateIn &s = k.s;
  AnchoredUpdateOut &o = k.o;
  sg.in(s.q, B * 96); sg.in(s.qd, B * 96); sg.in(s.quat, B * 32); sg.in(s.linvel, B * 24); sg.in(s.angvel, B * 24);
  sg.in(s.pos, B * 24); sg.in(s.stance, B * 4); sg.in(s.report, B * 4); sg.in(s.plane, B * 32);
  sg.in(s.heights, hf ? (size_t)hf->nx * (size_t)hf->ny * 8 : 0);
  sg.out(o.next, B * 4, keep); sg.out(o.sensor, B * 4, keep); sg.out(o.events, B * 4, keep); sg.out(o.gap, B * 32, keep);
  sg.out(o.normal, B * 96, keep); sg.out(o.fpos, B * 96, keep); sg.out(o.fvel, B * 96, keep); sg.out(o.status, B * 4);
  sg.inout(o.anchor, B * 96);
}

} // namespace rt
} // namespace qlamd
