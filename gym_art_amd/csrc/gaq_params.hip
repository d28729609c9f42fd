// gaq_params.hip -- the per-env parameter pipeline of libgaq: host models in and out (gaq_set_params*, gaq_get_params), the device sampler
// (gaq_set_randomizer, gaq_randomize_dev, gaq_set_param_trees, gaq_get_param_trees: quad_params_dev.hpp's sampler + QuadLink + update_model
// per env), staged per-episode re-randomisation with its refill pass, the inverse jacobians of Mellinger, and the per-env parameter flags
// whose counts feed the kernel selection.  The env core (gaq.hip) owns DevPtrs, allocates and frees par / jinv / traj, and calls in here
// for derive_model / inverse_jacobian / check_model and the passes a step launch or gaq_set_counters needs (gaq_host.hpp); this unit calls
// the core for refresh_feature_flags, fail, sync_handle and check_overrun.
#include "gaq_host.hpp"

namespace {

dim3 grid_for(int64_t count) { return dim3((unsigned)((count + kBlock - 1) / kBlock)); }   // 1-D launches of kBlock threads

// update_dynamics builds a NEW QuadrotorDynamics (quadrotor.py:857): since_last_svd = 0 (:104) and a fresh OUNoise (:198)
// for the envs whose parameters were replaced: env idx[k], or first + k when idx is null
__global__ __launch_bounds__(kBlock) void clear_dynamics_kernel(DevPtrs p, const int64_t* __restrict__ idx, int64_t first, int64_t count) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= count) return;
  const int64_t i = idx ? idx[k] : first + k;
  p.ctr[i] &= 0xFFFFu;
  float* ou = p.ou + (i / kTile) * (4 * kTile) + (i % kTile);
#pragma unroll
  for (int j = 0; j < 4; ++j) ou[j * kTile] = 0.0f;
}

// ---- parameter pipeline on the device (quad_params_dev.hpp): sampler + QuadLink + update_model per env ---------------
// [ntiles*64] the resample count at which ALL 45 planes of an env were last written: the fourth quarter of the traj | rcount | rz_flag
// allocation (the step kernels' buffer resource covers the first three)
__device__ __forceinline__ uint32_t* pfull_of(const DevPtrs& p) { return p.traj + 3 * p.ntiles * kTile; }

// where one env's 45 plane values go: value of `plane` at base[plane * stride + lane]
struct PlaneDest { double* base; int lane, stride; };
// env i's planes of the tile-major parameter array
__device__ __forceinline__ PlaneDest env_planes(const DevPtrs& p, int64_t i) {
  return {const_cast<double*>(p.par) + (i / kTile) * (int64_t)(kPar * kTile), (int)(i % kTile), kTile};
}
// a row of [45] doubles, plane order: an env's row of par_next (its NEXT draw, staged while the env keeps flying its current planes; the step
// kernel moves the row into the planes when it promotes the env, and clears the counters then), or a scratch row of gaq_get_params
__device__ __forceinline__ PlaneDest plane_row(double* row) { return {row, 0, 1}; }

// the planes of one derived model, exactly what set_params_impl writes on the host path
__device__ __forceinline__ void write_model_planes(const PlaneDest& to, double dt, const gaq::DerivedModel& dm) {
  auto P = [&](int plane) -> double& { return to.base[plane * to.stride + to.lane]; };
  P(PP_MASS) = dm.mass; P(PP_INV_MASS) = 1.0 / dm.mass;
#pragma unroll
  for (int j = 0; j < 3; ++j) { P(PP_INERTIA + j) = dm.inertia[j]; P(PP_INV_INERTIA + j) = 1.0 / dm.inertia[j]; }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    P(PP_THRUST_MAX + j) = dm.thrust_max[j]; P(PP_TORQUE_MAX + j) = dm.torque_max[j];
    P(PP_PROP_X + j) = dm.prop_pos[3 * j]; P(PP_PROP_Y + j) = dm.prop_pos[3 * j + 1]; P(PP_PROP_Z + j) = dm.prop_pos[3 * j + 2];
  }
  P(PP_TAU_UP) = 4 * dt / (dm.damp_time_up + 1e-6); P(PP_TAU_DOWN) = 4 * dt / (dm.damp_time_down + 1e-6);   // quadrotor.py:284-285
  P(PP_T_UP) = dm.damp_time_up; P(PP_T_DOWN) = dm.damp_time_down;
  P(PP_LINEARITY) = dm.linearity; P(PP_ARM) = dm.arm; P(PP_VEL_DAMP) = dm.vel_damp; P(PP_DAMP_Q) = dm.damp_omega_quadratic;
  P(PP_C_DRAG) = dm.c_drag; P(PP_C_ROLL) = dm.c_roll;
  if (to.stride == 1) P(PP_OU_SIGMA) = (double)(float)dm.ou_sigma;                                        // (a double in a row)
  else reinterpret_cast<float*>(to.base + PP_OU_SIGMA * to.stride)[to.lane] = (float)dm.ou_sigma;           // fp32 plane
  // construction hints of the compact path: derive_tree formed torque_max and prop_pos.xy with these very operations
  P(PP_T2T) = dm.t2t; P(PP_MX) = dm.motor_x; P(PP_MY) = dm.motor_y; P(PP_COMX) = dm.com[0]; P(PP_COMY) = dm.com[1];
  P(PP_COMPACT_OK) = 1.0;
}

// after write_model_planes(env_planes(p, i)) for a model the env has not flown yet
__device__ __forceinline__ void planes_replaced(const DevPtrs& p, int64_t i) {
  // every plane of env i now belongs to its resample count (a hot-planes-only promotion in the step kernel moves 19 of the 45 and leaves
  // this word alone: count != pfull then says "the other 26 are a draw behind", gaq_get_params)
  pfull_of(p)[i] = p.rcount[i];
  // a new QuadrotorDynamics: since_last_svd = 0 (quadrotor.py:104) and a fresh OUNoise (:198)
  p.ctr[i] &= 0xFFFFu;
  float* ou = p.ou + (i / kTile) * (4 * kTile) + (i % kTile);
#pragma unroll
  for (int j = 0; j < 4; ++j) ou[j * kTile] = 0.0f;
}

// the tree of env i at draw index k, a function of (seed, global env index, k) and the randomizer's settings
__device__ __forceinline__ void tree_at_draw(const StepCfg& cfg, const Randomizer& rz, int64_t i, uint32_t k, gaq::ParamTree& t) {
  if (rz.sampler == 2) gaq::random_quad_tree(cfg.seed, cfg.env_offset + (uint64_t)i, k, t);
  else gaq::perturb_tree(rz.base, rz.ratio, rz.sampler, cfg.seed, cfg.env_offset + (uint64_t)i, k, t);
}
// the tree env i flies with at resample count rc: its last draw, the base while it has never been drawn
__device__ __forceinline__ void tree_of_count(const StepCfg& cfg, const Randomizer& rz, int64_t i, uint32_t rc, gaq::ParamTree& t) {
  if (rc == 0) t = rz.base;
  else tree_at_draw(cfg, rz, i, rc - 1, t);
}

// The refill pass of dynamics_randomize_every (quadrotor.py:1063-1066 per env).  The step kernel PROMOTES a finished, due env to the planes
// staged for it in par_next and flags it; this pass derives the following draw (index = the env's resample count) into par_next for every
// flagged env.  Nothing waits for it: an env needs its staged planes only when its next episode ends, so the pass runs every
// min(64, ep_len + 1) steps (launch_step) instead of between every two step launches, where one lane's ~6000-instruction derivation was
// 27 us of pure latency (122 -> ~95 us per step with every episode of 2^20 staggered envs re-randomised).
__global__ __launch_bounds__(kBlock) void params_refill_kernel(DevPtrs p, StepCfg cfg, Randomizer rz) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= p.n) return;
  const uint32_t promoted = p.rz_flag[i];
  if (!promoted) return;
  if (promoted > 1u) atomicAdd(p.rz_overrun, promoted - 1u);      // consumed planes that were one draw old: must not happen
  gaq::ParamTree t;
  tree_at_draw(cfg, rz, i, p.rcount[i], t);
  gaq::DerivedModel dm;
  gaq::derive_tree(t, dm, rz.sampler == 2);
  write_model_planes(plane_row(p.par_next + i * (int64_t)kPar), cfg.dt, dm);
  p.rz_flag[i] = 0;
}

// gaq_randomize_dev: now, for the envs of `sel` (null = all): current planes = the next draw, and the env is flagged for the refill pass
__global__ __launch_bounds__(kBlock) void params_redraw_kernel(DevPtrs p, StepCfg cfg, Randomizer rz, const uint8_t* __restrict__ sel) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= p.n) return;
  if (!(sel == nullptr || sel[i] != 0)) return;
  const uint32_t rc = p.rcount[i];
  p.rcount[i] = rc + 1u;
  gaq::ParamTree t;
  tree_at_draw(cfg, rz, i, rc, t);
  gaq::DerivedModel dm;
  gaq::derive_tree(t, dm, rz.sampler == 2);
  write_model_planes(env_planes(p, i), cfg.dt, dm);
  planes_replaced(p, i);
  if (p.rz_every > 0) p.rz_flag[i] = 1u;  // its staged planes are one draw behind now
}

// Every env's planes rebuilt from its resample count (gaq_set_counters), or with `only_stale` those whose planes in memory are behind the
// count (envs promoted with the hot planes only since their last full write).  The current planes are those of the env's LAST draw; the
// env goes on flying it, so its SVD counter and OU state stay.
__global__ __launch_bounds__(kBlock) void params_rebuild_kernel(DevPtrs p, StepCfg cfg, Randomizer rz, bool only_stale) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= p.n) return;
  const uint32_t rc = p.rcount[i];
  if (only_stale && rc == pfull_of(p)[i]) return;
  if (rc == 0 && rz.sampler == 2) { pfull_of(p)[i] = 0u; return; }      // never drawn: the planes the handle was given stay
  gaq::ParamTree t;
  tree_of_count(cfg, rz, i, rc, t);
  gaq::DerivedModel dm;
  gaq::derive_tree(t, dm, rz.sampler == 2);
  write_model_planes(env_planes(p, i), cfg.dt, dm);
  pfull_of(p)[i] = rc;
  if (p.rz_every > 0) p.rz_flag[i] = 1u;
}

// gaq_get_params: a READ, nothing of the handle is touched.  rows_out[k][kPar] = the full plane row of env first + k's last draw where the
// planes in memory are behind it (hot-planes-only promotions: the count is past the last full write, so it is not zero); PP_COMPACT_OK = -1
// says "every plane in memory is current" (never drawn, or written whole)
__global__ __launch_bounds__(kBlock) void params_rows_kernel(DevPtrs p, StepCfg cfg, Randomizer rz, double* __restrict__ rows_out,
                                                             int64_t first, int64_t count) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= count) return;
  const int64_t i = first + k;
  const uint32_t rc = p.rcount[i];
  double* row = rows_out + k * (int64_t)kPar;
  if (rc == pfull_of(p)[i]) { row[PP_COMPACT_OK] = -1.0; return; }
  gaq::ParamTree t;
  tree_at_draw(cfg, rz, i, rc - 1, t);
  gaq::DerivedModel dm;
  gaq::derive_tree(t, dm, rz.sampler == 2);
  write_model_planes(plane_row(row), cfg.dt, dm);
}

// gaq_get_param_trees: no state is touched, the tree of env first + k's LAST resample is written out
__global__ __launch_bounds__(kBlock) void params_trees_kernel(DevPtrs p, StepCfg cfg, Randomizer rz, double* __restrict__ trees_out,
                                                              int64_t first, int64_t count) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= count) return;
  gaq::ParamTree t;
  tree_of_count(cfg, rz, first + k, p.rcount[first + k], t);
  for (int j = 0; j < gaq::TL_COUNT; ++j) trees_out[k * gaq::TL_COUNT + j] = t.v[j];
}

// Mellinger on per-env models whose parameters the DEVICE samples: the inverse jacobian of env i (quadrotor_control.py:192-203, :290-291)
// from the parameter planes the step kernels fly with (load_model: the compact construction included), for every env or for those that
// finished in the step launch just before (`done`: the only ones a launch can have promoted to new planes).  The same Gauss-Jordan
// elimination as the host's inverse_jacobian; thrust_max / mass is taken as thrust_max * (1 / mass) -- the plane the kernels read.
__global__ __launch_bounds__(kBlock) void jinv_kernel(DevPtrs p, StepCfg cfg, Model<double> um, const uint8_t* __restrict__ done) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= p.n || !p.jinv) return;
  if (done && !done[i]) return;
  Model<double> m;
  load_model<gaq::F_PER_ENV>(p, cfg, i / kTile, (uint32_t)(i % kTile), um, m);
  double J[4][8];
  const double ccw[4] = {-1, 1, -1, 1};
  for (int c = 0; c < 4; ++c) {
    J[0][c] = m.thrust_max[c] * m.inv_mass;
    J[1][c] = m.inv_inertia[0] * (m.thrust_max[c] * m.prop_y[c]);
    J[2][c] = m.inv_inertia[1] * (m.thrust_max[c] * -m.prop_x[c]);
    J[3][c] = m.inv_inertia[2] * (m.torque_max[c] * ccw[c]);
    for (int r = 0; r < 4; ++r) J[r][4 + c] = (r == c) ? 1.0 : 0.0;
  }
  for (int col = 0; col < 4; ++col) {
    int piv = col;
    for (int r = col + 1; r < 4; ++r) if (fabs(J[r][col]) > fabs(J[piv][col])) piv = r;
    for (int c = 0; c < 8; ++c) { const double t = J[col][c]; J[col][c] = J[piv][c]; J[piv][c] = t; }
    const double inv = 1.0 / J[col][col];      // (a singular jacobian gives non-finite controls: the NaN guard of the step reports it)
    for (int c = 0; c < 8; ++c) J[col][c] *= inv;
    for (int r = 0; r < 4; ++r) if (r != col) {
      const double f = J[r][col];
      for (int c = 0; c < 8; ++c) J[r][c] -= f * J[col][c];
    }
  }
  double* out = const_cast<double*>(p.jinv) + i * 16;
  for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) out[4 * r + c] = J[r][4 + c];
}

// caller-chosen trees [count][40] for envs first .. first+count-1: QuadLink + update_model on the device (no sampling)
__global__ __launch_bounds__(kBlock) void derive_trees_kernel(DevPtrs p, StepCfg cfg, const double* __restrict__ trees, int by_density,
                                                               int64_t first, int64_t count) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= count) return;
  gaq::ParamTree t;
  for (int j = 0; j < gaq::TL_COUNT; ++j) t.v[j] = trees[k * gaq::TL_COUNT + j];
  gaq::DerivedModel dm;
  gaq::derive_tree(t, dm, by_density != 0);
  write_model_planes(env_planes(p, first + k), cfg.dt, dm);
  planes_replaced(p, first + k);
}

}  // namespace

// ---- host side.  Declared in gaq_host.hpp, what the env core calls: the three model helpers, the three passes a step launch can need and
// the rebuild of gaq_set_counters ----
void derive_model(const gaq_model& g, double dt, Model<double>& m) {
  m.mass = g.mass; m.inv_mass = 1.0 / g.mass;
  for (int j = 0; j < 3; ++j) { m.inertia[j] = g.inertia[j]; m.inv_inertia[j] = 1.0 / g.inertia[j]; }
  for (int j = 0; j < 4; ++j) {
    m.thrust_max[j] = g.thrust_max[j]; m.torque_max[j] = g.torque_max[j];
    m.prop_x[j] = g.prop_pos[3 * j]; m.prop_y[j] = g.prop_pos[3 * j + 1]; m.prop_z[j] = g.prop_pos[3 * j + 2];
  }
  m.tau_up = 4 * dt / (g.damp_time_up + 1e-6);      // quadrotor.py:284-285
  m.tau_down = 4 * dt / (g.damp_time_down + 1e-6);
  m.linearity = g.linearity; m.arm = g.arm; m.vel_damp = g.vel_damp; m.damp_omega_q = g.damp_omega_quadratic;
  m.c_drag = g.c_drag; m.c_roll = g.c_roll; m.ou_sigma = (float)g.ou_sigma;
  m.jinv = nullptr;
}

// quadrotor_jacobian (quadrotor_control.py:192-203) and its inverse (:290-291), Gauss-Jordan with partial pivoting in fp64
bool inverse_jacobian(const gaq_model& g, double out[16]) {
  double J[4][8];
  const double ccw[4] = {-1, 1, -1, 1};
  for (int c = 0; c < 4; ++c) {
    J[0][c] = g.thrust_max[c] / g.mass;
    J[1][c] = (1.0 / g.inertia[0]) * (g.thrust_max[c] * g.prop_pos[3 * c + 1]);
    J[2][c] = (1.0 / g.inertia[1]) * (g.thrust_max[c] * -g.prop_pos[3 * c]);
    J[3][c] = (1.0 / g.inertia[2]) * (g.torque_max[c] * ccw[c]);
    for (int r = 0; r < 4; ++r) J[r][4 + c] = (r == c) ? 1.0 : 0.0;
  }
  for (int col = 0; col < 4; ++col) {
    int piv = col;
    for (int r = col + 1; r < 4; ++r) if (std::fabs(J[r][col]) > std::fabs(J[piv][col])) piv = r;
    if (std::fabs(J[piv][col]) < 1e-300) return false;
    for (int c = 0; c < 8; ++c) std::swap(J[col][c], J[piv][c]);
    const double inv = 1.0 / J[col][col];
    for (int c = 0; c < 8; ++c) J[col][c] *= inv;
    for (int r = 0; r < 4; ++r) if (r != col) {
      const double f = J[r][col];
      for (int c = 0; c < 8; ++c) J[r][c] -= f * J[col][c];
    }
  }
  for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) out[4 * r + c] = J[r][4 + c];
  return true;
}

int check_model(const gaq_model& g) {
  if (!(g.mass > 0) || !(g.inertia[0] > 0) || !(g.inertia[1] > 0) || !(g.inertia[2] > 0))
    return fail(GAQ_ERR_INVALID, "model: mass and inertia must be positive");
  if (g.damp_time_up < 0 || g.damp_time_down < 0) return fail(GAQ_ERR_INVALID, "model: negative motor time constant");
  return GAQ_OK;
}

// the refill pass of the staged parameter planes, on the stream of the step launches
int launch_refill(gaq_env* e, hipStream_t st) {
  hipLaunchKernelGGL(params_refill_kernel, grid_for(e->d.n), dim3(kBlock), 0, st, e->d, e->sc, e->rz);
  HIP_TRY(hipGetLastError());
  e->rz_since_refill = 0; e->rz_refill_now = false;
  return GAQ_OK;
}

// Mellinger with device-sampled per-env models: bring the inverse jacobians up to the parameter planes (jinv_kernel), on the stream that
// changed them
int launch_jinv(gaq_env* e, hipStream_t st, const uint8_t* done) {
  if (!e->d.jinv || !e->dev_params) return GAQ_OK;
  hipLaunchKernelGGL(jinv_kernel, grid_for(e->d.n), dim3(kBlock), 0, st, e->d, e->sc, e->um, done);
  HIP_TRY(hipGetLastError());
  return GAQ_OK;
}

static int launch_rebuild(gaq_env* e, hipStream_t st, bool only_stale) {
  hipLaunchKernelGGL(params_rebuild_kernel, grid_for(e->d.n), dim3(kBlock), 0, st, e->d, e->sc, e->rz, only_stale);
  HIP_TRY(hipGetLastError());
  return GAQ_OK;
}

// before a step launch whose promotions move all 45 planes and say nothing about the env's earlier ones: bring the envs that hot-only
// promotions left behind up to date (rare: the parameter flags changed under a live randomizer)
int launch_catch_up(gaq_env* e, hipStream_t st) {
  if (int rc = launch_rebuild(e, st, true)) return rc;
  e->rz_refill_now = true;
  e->cold_stale = false;
  return GAQ_OK;
}

// gaq_set_counters with a randomizer installed: the parameters are a function of (seed, global env index, resample count): rebuild them,
// then the inverse jacobians and the staged planes
int rebuild_params(gaq_env* e) {
  if (int rc = launch_rebuild(e, e->stream, false)) return rc;
  if (int rc = launch_jinv(e, e->stream, nullptr)) return rc;
  if (e->d.rz_every > 0) { if (int rc = launch_refill(e, e->stream)) return rc; }
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->cold_stale = false;      // (every env's planes were written whole)
  return GAQ_OK;
}

namespace {

// Does this model follow the reference's construction?  torque_max = t2t * thrust_max (quadrotor.py:176) for one t2t,
// and prop_pos.xy = (sx mx - comx, sy my - comy) with the sign pattern of inertia.py:238-240.  The hints are searched
// within an ulp of the obvious candidates and accepted only if they give back the model's numbers bit for bit.
bool find_construction(const Model<double>& m, double hint[5]) {
  auto same = [](double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0 || (a == 0.0 && b == 0.0); };
  auto around = [](double v, double out[3]) { out[0] = v; out[1] = std::nextafter(v, -INFINITY); out[2] = std::nextafter(v, INFINITY); };
  bool ok = false;
  if (m.thrust_max[0] != 0.0) {
    double cand[3]; around(m.torque_max[0] / m.thrust_max[0], cand);
    for (double t : cand) {
      bool all = true;
      for (int j = 0; j < 4; ++j) all = all && same(t * m.thrust_max[j], m.torque_max[j]);
      if (all) { hint[0] = t; ok = true; break; }
    }
  }
  if (!ok) return false;
  const double sx[4] = {1.0, -1.0, -1.0, 1.0}, sy[4] = {-1.0, -1.0, 1.0, 1.0};
  auto axis = [&](const double p[4], const double sgn[4], double& mo, double& co) {
    // p[j] = sgn[j] * mo - co:  with a = value at sgn = +1, b = value at sgn = -1:  mo ~ (a - b) / 2, co ~ -(a + b) / 2
    double a = 0, b = 0;
    for (int j = 0; j < 4; ++j) (sgn[j] > 0 ? a : b) = p[j];
    double mc[3], cc[3]; around((a - b) * 0.5, mc); around(-(a + b) * 0.5, cc);
    for (double mm : mc) for (double c : cc) {
      bool all = true;
      for (int j = 0; j < 4; ++j) all = all && same(sgn[j] * mm - c, p[j]);
      if (all) { mo = mm; co = c; return true; }
    }
    return false;
  };
  return axis(m.prop_x, sx, hint[1], hint[3]) && axis(m.prop_y, sy, hint[2], hint[4]);
}

// flag byte of env i (ParamFlag bits); the handle-wide counts move by the difference, so nothing ever scans all envs
void set_env_flags(gaq_env* e, int64_t i, uint8_t nf) {
  const uint8_t of = e->pflags[(size_t)i];
  auto moved = [&](uint8_t bit) { return (int)((nf & bit) != 0) - (int)((of & bit) != 0); };
  e->cnt_lag += moved(PF_LAG); e->cnt_drag += moved(PF_DRAG); e->cnt_noncompact += moved(PF_NONCOMPACT); e->cnt_damp += moved(PF_DAMP);
  e->pflags[(size_t)i] = nf;
}
// kernel selection of the handle from the running counts
void flags_from_counts(gaq_env* e) {
  e->any_lag = e->cnt_lag > 0; e->any_drag = e->cnt_drag > 0;
  e->sc.compact_params = (e->cnt_noncompact == 0 && !getenv("GAQ_NO_COMPACT")) ? 1 : 0;
  e->sc.zero_damp = (e->cnt_damp == 0 && !getenv("GAQ_NO_COMPACT")) ? 1 : 0;
  refresh_feature_flags(e);
}
// what a parameter tree brings (its derived planes always follow the compact construction)
uint8_t tree_flags(const gaq_quad_params& t, double dt) {
  return param_flags(4 * dt / (t.motor[9] + 1e-6), 4 * dt / (t.motor[10] + 1e-6), t.motor[7], t.motor[8], true, t.damp[0], t.damp[1]);
}

// The plane that holds double k of a gaq_model as it is, for the host path in both directions (set_params_impl, gaq_get_params).  Not in
// the list: the derived planes (inverses, tau, construction hints); PP_OU_SIGMA is an fp32 plane, which both handle themselves.
constexpr int kModelPlane[GAQ_MODEL_NUM_DOUBLES] = {
    PP_MASS, PP_INERTIA, PP_INERTIA + 1, PP_INERTIA + 2,
    PP_THRUST_MAX, PP_THRUST_MAX + 1, PP_THRUST_MAX + 2, PP_THRUST_MAX + 3, PP_TORQUE_MAX, PP_TORQUE_MAX + 1, PP_TORQUE_MAX + 2, PP_TORQUE_MAX + 3,
    PP_PROP_X, PP_PROP_Y, PP_PROP_Z, PP_PROP_X + 1, PP_PROP_Y + 1, PP_PROP_Z + 1, PP_PROP_X + 2, PP_PROP_Y + 2, PP_PROP_Z + 2,
    PP_PROP_X + 3, PP_PROP_Y + 3, PP_PROP_Z + 3,
    PP_T_UP, PP_T_DOWN, PP_LINEARITY, PP_ARM, PP_OU_SIGMA, PP_VEL_DAMP, PP_DAMP_Q, PP_C_DRAG, PP_C_ROLL};
static_assert(sizeof(gaq_model) == GAQ_MODEL_NUM_DOUBLES * sizeof(double) && offsetof(gaq_model, ou_sigma) == 28 * sizeof(double), "gaq_model layout");

int check_range(const gaq_env* e, int64_t first, int64_t count) {
  if (first < 0 || count < 0 || first + count > e->d.n) return fail(GAQ_ERR_INVALID, "env range out of bounds");
  return GAQ_OK;
}

// shared by gaq_set_params / gaq_set_params_indexed: `idx` == nullptr means envs first .. first+count-1
int set_params_impl(gaq_env* e, const gaq_model* models, const int64_t* idx, int64_t first, int64_t count) {
  if (!e || !models) return fail(GAQ_ERR_INVALID, "null argument");
  e->info_valid = false;
  if (!e->cfg.per_env_params) return fail(GAQ_ERR_STATE, "handle was created with per_env_params = 0");
  if (e->dev_params) return fail(GAQ_ERR_STATE, "this handle's parameters are managed on the device (gaq_set_randomizer / "
                                                "gaq_set_param_trees): gaq_set_params is not available");
  if (count < 0) return fail(GAQ_ERR_INVALID, "negative count");
  if (count == 0) return GAQ_OK;
  auto env_of = [&](int64_t k) { return idx ? idx[k] : first + k; };
  int64_t lo = e->d.n, hi = -1;
  for (int64_t k = 0; k < count; ++k) {
    const int64_t i = env_of(k);
    if (i < 0 || i >= e->d.n) return fail(GAQ_ERR_INVALID, "env index out of bounds");
    lo = i < lo ? i : lo; hi = i > hi ? i : hi;
  }
  HIP_TRY(hipSetDevice(e->cfg.device));
  double* hp = e->host_par.data();
  std::vector<double> ji(e->d.jinv ? (size_t)count * 16 : 0);
  for (int64_t k = 0; k < count; ++k) {
    if (check_model(models[k]) != GAQ_OK) return GAQ_ERR_INVALID;
    if (e->d.jinv && !inverse_jacobian(models[k], ji.data() + (size_t)k * 16)) return fail(GAQ_ERR_INVALID, "singular quadrotor jacobian");
  }
  for (int64_t k = 0; k < count; ++k) {
    Model<double> m;
    derive_model(models[k], e->sc.dt, m);
    const int64_t i = env_of(k);
    auto P = [&](int plane) -> double& { return hp[tidx(i, kPar, plane)]; };
    const double* field = reinterpret_cast<const double*>(&models[k]);
    for (int f = 0; f < GAQ_MODEL_NUM_DOUBLES; ++f) if (kModelPlane[f] != PP_OU_SIGMA) P(kModelPlane[f]) = field[f];
    P(PP_INV_MASS) = m.inv_mass;
    for (int j = 0; j < 3; ++j) P(PP_INV_INERTIA + j) = m.inv_inertia[j];
    P(PP_TAU_UP) = m.tau_up; P(PP_TAU_DOWN) = m.tau_down;
    reinterpret_cast<float*>(hp + tidx(i - i % kTile, kPar, PP_OU_SIGMA))[i % kTile] = (float)models[k].ou_sigma;   // fp32 plane
    // construction hints: accepted only when they reproduce the given numbers bit for bit
    double hint[5] = {0, 0, 0, 0, 0};
    const bool compact_ok = find_construction(m, hint);
    P(PP_COMPACT_OK) = compact_ok ? 1.0 : 0.0;
    for (int j = 0; j < 5; ++j) P(PP_T2T + j) = hint[j];
    // flag byte of this env; the handle-wide counts move by the difference (no scan over all envs)
    set_env_flags(e, i, param_flags(m.tau_up, m.tau_down, m.c_drag, m.c_roll, compact_ok, m.vel_damp, m.damp_omega_q));
  }
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (int rc_ = sync_handle(e)) return rc_;
  if (e->d.jinv) {   // Mellinger: one inverse jacobian per env (quadrotor_control.py:290-291)
    if (!idx) {
      HIP_TRY(hipMemcpy(const_cast<double*>(e->d.jinv) + (size_t)first * 16, ji.data(), ji.size() * sizeof(double), hipMemcpyHostToDevice));
    } else {
      for (int64_t k = 0; k < count; ++k)
        HIP_TRY(hipMemcpy(const_cast<double*>(e->d.jinv) + (size_t)idx[k] * 16, ji.data() + (size_t)k * 16, 16 * sizeof(double), hipMemcpyHostToDevice));
    }
  }
  // upload the touched tiles only: runs of adjacent touched tiles go in one copy each (a contiguous range is one run)
  {
    std::vector<int64_t> tiles((size_t)count);
    for (int64_t k = 0; k < count; ++k) tiles[(size_t)k] = env_of(k) / kTile;
    std::sort(tiles.begin(), tiles.end());
    tiles.erase(std::unique(tiles.begin(), tiles.end()), tiles.end());
    for (size_t a = 0; a < tiles.size();) {
      size_t b = a + 1;
      while (b < tiles.size() && tiles[b] == tiles[b - 1] + 1) ++b;
      HIP_TRY(hipMemcpy(const_cast<double*>(e->d.par) + (size_t)tiles[a] * kPar * kTile, hp + (size_t)tiles[a] * kPar * kTile,
                        (b - a) * (size_t)kParBytes, hipMemcpyHostToDevice));
      a = b;
    }
  }
  // a new QuadrotorDynamics starts with since_last_svd = 0 and a fresh OUNoise (quadrotor.py:104, :198)
  Scratch di;   // the device's copy of idx
  if (idx) {
    if (di.alloc(sizeof(int64_t) * (size_t)count)) return GAQ_ERR_DEVICE;
    HIP_TRY(hipMemcpy(di.p, idx, sizeof(int64_t) * (size_t)count, hipMemcpyHostToDevice));
  }
  hipLaunchKernelGGL(clear_dynamics_kernel, grid_for(count), dim3(kBlock), 0, e->stream, e->d, (const int64_t*)di.p, first, count);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream));
  flags_from_counts(e);
  return GAQ_OK;
}

int need_device_params(gaq_env* e) {
  if (!e) return fail(GAQ_ERR_INVALID, "null handle");
  if (!e->cfg.per_env_params) return fail(GAQ_ERR_STATE, "handle was created with per_env_params = 0");
  return GAQ_OK;
}
int check_tree(const gaq_quad_params& t, bool by_density = false) {
  const double* v = reinterpret_cast<const double*>(&t);
  for (int k = 0; k < GAQ_TREE_DOUBLES; ++k) if (!std::isfinite(v[k])) return fail(GAQ_ERR_INVALID, "parameter tree: non-finite leaf");
  if (!by_density && !(t.body[3] + t.payload[3] + 4 * (t.arms[3] + t.motors[2] + t.propellers[2]) > 0))
    return fail(GAQ_ERR_INVALID, "parameter tree: total mass must be positive");
  if (t.motor[7] != 0.0 || t.motor[8] != 0.0)
    return fail(GAQ_ERR_INVALID, "parameter tree: rotor drag / rolling moment (C_drag, C_roll != 0) needs the generic kernel and the host path (gaq_set_params)");
  return GAQ_OK;
}

}  // namespace

extern "C" {

int gaq_set_params(gaq_env* e, const gaq_model* models, int64_t first, int64_t count) {
  if (e) { if (int rc = check_range(e, first, count)) return rc; }
  return set_params_impl(e, models, nullptr, first, count);
}

int gaq_set_params_indexed(gaq_env* e, const gaq_model* models, const int64_t* env_idx, int64_t count) {
  if (!env_idx) return fail(GAQ_ERR_INVALID, "null argument");
  return set_params_impl(e, models, env_idx, 0, count);
}

int gaq_set_randomizer(gaq_env* e, const gaq_randomizer* rz) {
  if (int rc = need_device_params(e)) return rc;
  e->info_valid = false;
  if (!rz) return fail(GAQ_ERR_INVALID, "null argument");
  if (rz->sampler < 0 || rz->sampler > 2 || rz->every < 0) return fail(GAQ_ERR_INVALID, "randomizer: unknown sampler / negative period");
  if (rz->every > 0 && !e->cfg.auto_reset)
    return fail(GAQ_ERR_INVALID, "randomizer: every > 0 (dynamics_randomize_every inside the step launch) needs auto_reset = 1 -- without it a "
                                 "finished env reports done on every step until the caller resets it; call gaq_randomize_dev(mask) then");
  if (rz->sampler != 2) { if (int rc = check_tree(rz->base)) return rc; }
  for (int k = 0; k < GAQ_TREE_DOUBLES; ++k) if (!std::isfinite(rz->ratio[k])) return fail(GAQ_ERR_INVALID, "randomizer: non-finite noise ratio");
  static_assert(sizeof(gaq::ParamTree) == sizeof(gaq_quad_params) && gaq::TL_COUNT == GAQ_TREE_DOUBLES, "parameter tree layout");
  HIP_TRY(hipSetDevice(e->cfg.device));
  if (int rc_ = sync_handle(e)) return rc_;
  e->rz.sampler = rz->sampler; e->rz.every = rz->every;
  std::memcpy(e->rz.ratio, rz->ratio, sizeof(e->rz.ratio));
  std::memcpy(&e->rz.base, &rz->base, sizeof(e->rz.base));
  e->rz_on = true; e->dev_params = true;
  if (rz->every > 0 && !e->d.par_next) {       // per-episode re-randomisation: staged planes of every env's NEXT draw + flags
    const size_t nt = (size_t)e->d.ntiles;
    // everything is allocated and filled BEFORE the handle's pointers change: an error on the way leaves the handle as it was
    Scratch both_, over_;                      // [par planes | skew | par_next rows] in one allocation; the overrun counter
    if (both_.alloc(2 * nt * kParBytes + kParNextSkew * sizeof(double)) || over_.alloc(sizeof(uint32_t))) return GAQ_ERR_DEVICE;
    double* both = (double*)both_.p;
    HIP_TRY(hipMemcpy(both, e->d.par, nt * kParBytes, hipMemcpyDeviceToDevice));
    HIP_TRY(hipMemset(both + nt * kPar * kTile, 0, nt * kParBytes + kParNextSkew * sizeof(double)));      // rows: filled by the first refill pass
    HIP_TRY(hipMemset(over_.p, 0, sizeof(uint32_t)));
    {   // nothing staged yet: the first refill pass derives every env's next draw
      std::vector<uint32_t> ones(nt * kTile, 1u);
      HIP_TRY(hipMemcpy(e->d.rz_flag, ones.data(), ones.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    (void)hipFree(const_cast<double*>(e->d.par));
    e->d.par = both;
    e->d.par_next = both + nt * kPar * kTile + kParNextSkew;
    e->d.rz_overrun = (uint32_t*)over_.p;
    both_.p = nullptr; over_.p = nullptr;      // owned by the handle now
  }
  e->d.rz_every = e->d.par_next ? rz->every : 0;
  e->rz_refill_now = true;
  // what the sampler can produce is known from the nominal model: a leaf that is zero stays zero (scale = |ratio/2 v|),
  // so lag / damping exist iff the base has them; the derived planes always follow the compact construction
  // (RandomQuad: motor time constants U(0.15, 0.2) s -> lag; no drag, no damping: quadrotor_randomization.py:211-229)
  const uint8_t nf = rz->sampler == 2 ? (uint8_t)PF_LAG : tree_flags(rz->base, e->sc.dt);
  for (int64_t i = 0; i < e->d.n; ++i) set_env_flags(e, i, nf);
  flags_from_counts(e);
  return GAQ_OK;
}

int gaq_randomize_dev(gaq_env* e, const uint8_t* mask_dev, void* stream) {
  if (int rc = need_device_params(e)) return rc;
  e->info_valid = false;
  if (!e->rz_on) return fail(GAQ_ERR_STATE, "no randomizer installed (gaq_set_randomizer)");
  HIP_TRY(hipSetDevice(e->cfg.device));
  e->user_stream = (hipStream_t)stream; e->user_stream_used = true;
  hipLaunchKernelGGL(params_redraw_kernel, grid_for(e->d.n), dim3(kBlock), 0, (hipStream_t)stream, e->d, e->sc, e->rz, mask_dev);
  HIP_TRY(hipGetLastError());
  if (int rc = launch_jinv(e, (hipStream_t)stream, nullptr)) return rc;
  if (e->d.rz_every > 0) return launch_refill(e, (hipStream_t)stream);      // the redrawn envs' staged planes: one draw further
  return GAQ_OK;
}

int gaq_set_param_trees(gaq_env* e, const gaq_quad_params* trees, int32_t links_by_density, int64_t first, int64_t count) {
  if (int rc = need_device_params(e)) return rc;
  e->info_valid = false;
  if (!trees) return fail(GAQ_ERR_INVALID, "null argument");
  if (int rc = check_range(e, first, count)) return rc;
  if (count == 0) return GAQ_OK;
  if (!e->dev_params && (e->cnt_lag | e->cnt_drag | e->cnt_noncompact | e->cnt_damp) != 0)
    return fail(GAQ_ERR_STATE, "this handle already holds host-supplied parameters (gaq_set_params): do not mix the two paths");
  for (int64_t k = 0; k < count; ++k) if (int rc = check_tree(trees[k], links_by_density != 0)) return rc;
  HIP_TRY(hipSetDevice(e->cfg.device));
  if (int rc_ = sync_handle(e)) return rc_;
  Scratch dt_;
  if (dt_.alloc(sizeof(gaq_quad_params) * (size_t)count)) return GAQ_ERR_DEVICE;
  HIP_TRY(hipMemcpy(dt_.p, trees, sizeof(gaq_quad_params) * (size_t)count, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(derive_trees_kernel, grid_for(count), dim3(kBlock), 0, e->stream, e->d, e->sc, (const double*)dt_.p, (int)links_by_density, first, count);
  HIP_TRY(hipGetLastError());
  e->dev_params = true;
  if (int rc = launch_jinv(e, e->stream, nullptr)) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (int64_t k = 0; k < count; ++k) set_env_flags(e, first + k, tree_flags(trees[k], e->sc.dt));
  flags_from_counts(e);
  return GAQ_OK;
}

int gaq_get_params(gaq_env* e, gaq_model* out, int64_t first, int64_t count) {
  if (!e || !out) return fail(GAQ_ERR_INVALID, "null argument");
  if (!e->cfg.per_env_params) return fail(GAQ_ERR_STATE, "handle was created with per_env_params = 0");
  if (int rc = check_range(e, first, count)) return rc;
  if (count == 0) return GAQ_OK;
  HIP_TRY(hipSetDevice(e->cfg.device));
  if (int rc_ = sync_handle(e)) return rc_;
  if (int rc_ = check_overrun(e)) return rc_;
  // A READ: nothing of the handle changes.  Per-episode re-randomisation moves only the planes the step kernels read when it promotes an
  // env (gaq_kernels.hpp: kHotPlanes); for exactly those envs (resample count != the count of their last full write) the whole row is
  // derived afresh from (seed, global env index, count) into a scratch buffer -- only the envs asked for, whatever the randomizer's
  // period is NOW (gaq_set_randomizer(every = 0) after a period of promotions leaves the stale planes stale)
  std::vector<double> rows;
  if (e->rz_on && e->cold_stale) {
    Scratch rs_;
    if (rs_.alloc(sizeof(double) * (size_t)count * kPar)) return GAQ_ERR_DEVICE;
    hipLaunchKernelGGL(params_rows_kernel, grid_for(count), dim3(kBlock), 0, e->stream, e->d, e->sc, e->rz, (double*)rs_.p, first, count);
    HIP_TRY(hipGetLastError());
    rows.resize((size_t)count * kPar);
    HIP_TRY(hipMemcpyAsync(rows.data(), rs_.p, rows.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
  }
  const int64_t t0 = first / kTile, t1 = (first + count - 1) / kTile + 1;
  std::vector<double> buf((size_t)(t1 - t0) * kPar * kTile);
  HIP_TRY(hipMemcpy(buf.data(), e->d.par + (size_t)t0 * kPar * kTile, buf.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (int64_t k = 0; k < count; ++k) {
    const int64_t i = first + k - t0 * kTile;
    const double* row = (!rows.empty() && rows[(size_t)k * kPar + PP_COMPACT_OK] > 0.0) ? &rows[(size_t)k * kPar] : nullptr;
    auto P = [&](int plane) { return row ? row[plane] : buf[tidx(i, kPar, plane)]; };
    double* field = reinterpret_cast<double*>(&out[k]);
    for (int f = 0; f < GAQ_MODEL_NUM_DOUBLES; ++f) field[f] = P(kModelPlane[f]);
    if (!row) out[k].ou_sigma = (double)reinterpret_cast<const float*>(&buf[tidx(i - i % kTile, kPar, PP_OU_SIGMA)])[i % kTile];   // fp32 plane
  }
  return GAQ_OK;
}

int gaq_get_param_trees(gaq_env* e, gaq_quad_params* out, int64_t first, int64_t count) {
  if (int rc = need_device_params(e)) return rc;
  if (!out) return fail(GAQ_ERR_INVALID, "null argument");
  if (!e->rz_on) return fail(GAQ_ERR_STATE, "no randomizer installed (gaq_set_randomizer): the sampled trees are a function of its settings");
  if (int rc = check_range(e, first, count)) return rc;
  if (count == 0) return GAQ_OK;
  HIP_TRY(hipSetDevice(e->cfg.device));
  if (int rc_ = sync_handle(e)) return rc_;
  Scratch dt_;
  if (dt_.alloc(sizeof(gaq_quad_params) * (size_t)count)) return GAQ_ERR_DEVICE;
  hipLaunchKernelGGL(params_trees_kernel, grid_for(count), dim3(kBlock), 0, e->stream, e->d, e->sc, e->rz, (double*)dt_.p, first, count);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, dt_.p, sizeof(gaq_quad_params) * (size_t)count, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GAQ_OK;
}

}  // extern "C"
