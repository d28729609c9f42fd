// gaq_sharded.hip -- one batch over several devices in one process (include/gaq.h gaq_sharded).  It drives its shards, ordinary gaq_env
// handles, through the public C ABI; of the env core's internals (gaq_host.hpp) it reads a few fields of the handle and calls sync_handle and
// check_overrun.
#include "gaq_host.hpp"

// ---- one batch over several devices, one process (include/gaq.h: gaq_sharded) --------------------------------------------------
// Shard k is an ordinary gaq_env on device dev[k] holding the global envs [first[k], first[k] + count[k]).  A call records an event on
// the caller's stream (device dev[0]), every REMOTE shard's own stream waits for it, pulls its slice of the inputs over with a peer
// copy, launches its step and pushes its slices of obs / reward / done back; shards that live on dev[0] run on the caller's stream and
// read / write the caller's tensors in place; finally the caller's stream waits for the remote shards' events.  Nothing blocks the host.
struct gaq_sharded {
  struct Shard {
    gaq_env* env = nullptr;
    int64_t first = 0, count = 0;
    int dev = 0;
    bool direct = false;             // lives on the root device: steps on the caller's stream, straight on the caller's tensors
    hipStream_t st = nullptr;        // remote shards: their own stream ...
    hipEvent_t ev = nullptr;         // ... and the event the caller's stream waits for
    float* act = nullptr; float* obs = nullptr; float* rew = nullptr; uint8_t* done = nullptr; uint8_t* mask = nullptr;   // on dev
  };
  std::vector<Shard> sh;
  bool owns = false;
  int root = 0;
  int64_t n = 0;
  int D = 18;
  hipEvent_t start = nullptr;        // on the root device: "the caller's inputs are ready"
  hipStream_t root_stream = nullptr; // host-pointer forms
  char* stage = nullptr;             // [actions 16n | reward 4n | done n | mask n | obs 4 D n] on the root device
  size_t off_rew = 0, off_done = 0, off_mask = 0, off_obs = 0;
};

namespace {

struct DeviceGuard {                 // the caller's current device is the caller's business (torch keeps its own idea of it)
  int prev = -1;
  DeviceGuard() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

int shard_range_impl(int64_t n, int32_t K, int32_t k, int32_t align, int64_t* first, int64_t* count) {
  if (n <= 0 || K <= 0 || k < 0 || k >= K || align <= 0) return fail(GAQ_ERR_INVALID, "gaq_shard_range: bad argument");
  int64_t a = kTile, b = align;
  while (b) { const int64_t t = a % b; a = b; b = t; }              // gcd
  const int64_t unit = (int64_t)kTile / a * align;                   // whole tiles AND whole worlds
  const int64_t units = (n + unit - 1) / unit;
  const int64_t base = units / K, extra = units % K;
  int64_t f = ((int64_t)k * base + (k < extra ? k : extra)) * unit;
  int64_t l = f + (base + (k < extra ? 1 : 0)) * unit;
  if (f > n) f = n;
  if (l > n) l = n;
  *first = f; *count = l - f;
  return GAQ_OK;
}

void free_sharded(gaq_sharded* s) {
  if (!s) return;
  for (auto& x : s->sh) {
    if (hipSetDevice(x.dev) != hipSuccess) continue;
    if (x.st) { (void)hipStreamSynchronize(x.st); (void)hipStreamDestroy(x.st); }
    if (x.ev) (void)hipEventDestroy(x.ev);
    (void)hipFree(x.act); (void)hipFree(x.obs); (void)hipFree(x.rew); (void)hipFree(x.done); (void)hipFree(x.mask);
    if (s->owns && x.env) (void)gaq_destroy(x.env);
  }
  if (hipSetDevice(s->root) == hipSuccess) {
    if (s->root_stream) { (void)hipStreamSynchronize(s->root_stream); (void)hipStreamDestroy(s->root_stream); }
    if (s->start) (void)hipEventDestroy(s->start);
    (void)hipFree(s->stage);
  }
  delete s;
}

// streams, events and the remote shards' local buffers; s->sh[k].{env, first, count, dev} are filled in
int finish_sharded(gaq_sharded* s) {
  s->root = s->sh[0].dev;
  s->D = s->sh[0].env->obs_dim;
  s->n = 0;
  const bool force_copy = env_override("GAQ_SHARDED_FORCE_COPY") == 1;    // tests on a one-GPU box: every shard takes the remote path
  for (auto& x : s->sh) {
    if (x.env->obs_dim != s->D) return fail(GAQ_ERR_INVALID, "sharded: the shards' observation widths differ");
    if (x.first != s->n) return fail(GAQ_ERR_INVALID, "sharded: shard ranges must be consecutive");
    if ((int64_t)x.env->cfg.env_id_offset != s->sh[0].env->cfg.env_id_offset + x.first)
      return fail(GAQ_ERR_INVALID, "sharded: env_id_offset of every shard must continue the previous shard's global range");
    if (&x != &s->sh.back() && (x.count % kTile) != 0)
      return fail(GAQ_ERR_INVALID, "sharded: every shard but the last must hold a multiple of 64 envs (16-byte aligned slices)");
    s->n += x.count;
    x.direct = (x.dev == s->root) && !force_copy;
  }
  HIP_TRY(hipSetDevice(s->root));
  HIP_TRY(hipEventCreateWithFlags(&s->start, hipEventDisableTiming));
  HIP_TRY(hipStreamCreateWithFlags(&s->root_stream, hipStreamNonBlocking));
  for (auto& x : s->sh) {
    if (x.direct) continue;
    HIP_TRY(hipSetDevice(x.dev));
    if (x.dev != s->root) {            // best effort: with peer access the copies are direct xGMI DMA, without it the runtime stages them
      int can = 0;
      if (hipDeviceCanAccessPeer(&can, x.dev, s->root) == hipSuccess && can) { if (hipDeviceEnablePeerAccess(s->root, 0) != hipSuccess) (void)hipGetLastError(); }
      HIP_TRY(hipSetDevice(s->root));
      if (hipDeviceCanAccessPeer(&can, s->root, x.dev) == hipSuccess && can) { if (hipDeviceEnablePeerAccess(x.dev, 0) != hipSuccess) (void)hipGetLastError(); }
      HIP_TRY(hipSetDevice(x.dev));
    }
    HIP_TRY(hipStreamCreateWithFlags(&x.st, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&x.ev, hipEventDisableTiming));
    const size_t c = (size_t)x.count;
    HIP_TRY(hipMalloc((void**)&x.act, 16 * c));
    HIP_TRY(hipMalloc((void**)&x.obs, 4 * (size_t)s->D * c));
    HIP_TRY(hipMalloc((void**)&x.rew, 4 * c));
    HIP_TRY(hipMalloc((void**)&x.done, c));
    HIP_TRY(hipMalloc((void**)&x.mask, c));
  }
  return GAQ_OK;
}

hipError_t copy_between(void* dst, int dst_dev, const void* src, int src_dev, size_t bytes, hipStream_t st) {
  if (dst_dev == src_dev) return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st);
  return hipMemcpyPeerAsync(dst, dst_dev, src, src_dev, bytes, st);
}

// reset (actions == nullptr) or step of every shard; device pointers on the root device
int fan_out(gaq_sharded* s, const float* actions, const uint8_t* mask, float* obs, float* reward, uint8_t* done, hipStream_t ust) {
  const size_t D = (size_t)s->D;
  bool any_remote = false;
  for (auto& x : s->sh) any_remote = any_remote || !x.direct;
  if (any_remote) {
    HIP_TRY(hipSetDevice(s->root));
    HIP_TRY(hipEventRecord(s->start, ust));
    for (auto& x : s->sh) {
      if (x.direct) continue;
      const size_t f = (size_t)x.first, c = (size_t)x.count;
      HIP_TRY(hipSetDevice(x.dev));
      HIP_TRY(hipStreamWaitEvent(x.st, s->start, 0));
      int rc;
      if (actions) {
        HIP_TRY(copy_between(x.act, x.dev, actions + 4 * f, s->root, 16 * c, x.st));
        rc = gaq_step_dev(x.env, x.act, x.obs, x.rew, x.done, x.st);
      } else {
        if (mask) HIP_TRY(copy_between(x.mask, x.dev, mask + f, s->root, c, x.st));
        rc = gaq_reset_dev(x.env, mask ? x.mask : nullptr, x.obs, x.st);
      }
      if (rc) return rc;
      HIP_TRY(copy_between(obs + D * f, s->root, x.obs, x.dev, 4 * D * c, x.st));
      if (actions) {
        HIP_TRY(copy_between(reward + f, s->root, x.rew, x.dev, 4 * c, x.st));
        HIP_TRY(copy_between(done + f, s->root, x.done, x.dev, c, x.st));
      }
      HIP_TRY(hipEventRecord(x.ev, x.st));
    }
  }
  for (auto& x : s->sh) {              // the root device's own shards: on the caller's stream, in the caller's tensors
    if (!x.direct) continue;
    const size_t f = (size_t)x.first;
    const int rc = actions ? gaq_step_dev(x.env, actions + 4 * f, obs + D * f, reward + f, done + f, ust)
                           : gaq_reset_dev(x.env, mask ? mask + f : nullptr, obs + D * f, ust);
    if (rc) return rc;
  }
  if (any_remote) {
    HIP_TRY(hipSetDevice(s->root));
    for (auto& x : s->sh) if (!x.direct) HIP_TRY(hipStreamWaitEvent(ust, x.ev, 0));
  }
  return GAQ_OK;
}

int need_stage(gaq_sharded* s) {
  if (s->stage) return GAQ_OK;
  const size_t n = (size_t)s->n, D = (size_t)s->D;
  s->off_rew = (16 * n + 15) & ~(size_t)15;
  s->off_done = s->off_rew + 4 * n;
  s->off_mask = (s->off_done + n + 15) & ~(size_t)15;
  s->off_obs = (s->off_mask + n + 15) & ~(size_t)15;
  HIP_TRY(hipSetDevice(s->root));
  HIP_TRY(hipMalloc((void**)&s->stage, s->off_obs + 4 * D * n));
  return GAQ_OK;
}

}  // namespace

extern "C" {

int gaq_shard_range(int64_t n, int32_t num_shards, int32_t k, int32_t align, int64_t* first, int64_t* count) {
  if (!first || !count) return fail(GAQ_ERR_INVALID, "null argument");
  return shard_range_impl(n, num_shards, k, align, first, count);
}

int gaq_create_sharded(const gaq_config* cfg, const int32_t* device_ids, int32_t num_devices, gaq_sharded** out) {
  if (!cfg || !device_ids || !out) return fail(GAQ_ERR_INVALID, "null argument");
  if (num_devices <= 0 || num_devices > 64) return fail(GAQ_ERR_INVALID, "sharded: num_devices must be in [1, 64]");
  if (cfg->struct_size != sizeof(gaq_config) || cfg->abi_version != GAQ_ABI_VERSION)
    return fail(GAQ_ERR_INVALID, "gaq_config size/version mismatch (header vs library)");
  if (cfg->num_envs <= 0) return fail(GAQ_ERR_INVALID, "num_envs must be positive");
  const int nd = gaq_num_devices();
  if (nd <= 0) return fail(GAQ_ERR_DEVICE, "no HIP device visible: libgaq has no CPU fallback");
  for (int k = 0; k < num_devices; ++k)
    if (device_ids[k] < 0 || device_ids[k] >= nd) return fail(GAQ_ERR_INVALID, "sharded: device id out of range");
  DeviceGuard guard;
  gaq_sharded* s = new (std::nothrow) gaq_sharded();
  if (!s) return fail(GAQ_ERR_DEVICE, "out of host memory");
  s->owns = true;
  const int align = cfg->swarm.agents > 1 ? cfg->swarm.agents : 1;
  for (int k = 0; k < num_devices; ++k) {
    int64_t f = 0, c = 0;
    if (int rc = shard_range_impl(cfg->num_envs, num_devices, k, align, &f, &c)) { free_sharded(s); return rc; }
    if (c == 0) continue;                 // fewer tiles than devices: the tail devices stay idle
    gaq_config sc = *cfg;
    sc.num_envs = c; sc.env_id_offset = cfg->env_id_offset + f; sc.device = device_ids[k];
    gaq_env* e = nullptr;
    if (int rc = gaq_create(&sc, &e)) { free_sharded(s); return rc; }
    gaq_sharded::Shard x;
    x.env = e; x.first = f; x.count = c; x.dev = device_ids[k];
    s->sh.push_back(x);
  }
  if (int rc = finish_sharded(s)) { free_sharded(s); return rc; }
  *out = s;
  return GAQ_OK;
}

int gaq_sharded_from_handles(gaq_env* const* envs, int32_t num_shards, gaq_sharded** out) {
  if (!envs || !out) return fail(GAQ_ERR_INVALID, "null argument");
  if (num_shards <= 0 || num_shards > 64) return fail(GAQ_ERR_INVALID, "sharded: num_shards must be in [1, 64]");
  DeviceGuard guard;
  gaq_sharded* s = new (std::nothrow) gaq_sharded();
  if (!s) return fail(GAQ_ERR_DEVICE, "out of host memory");
  s->owns = false;
  int64_t f = 0;
  for (int k = 0; k < num_shards; ++k) {
    if (!envs[k]) { free_sharded(s); return fail(GAQ_ERR_INVALID, "null shard handle"); }
    gaq_sharded::Shard x;
    x.env = envs[k]; x.first = f; x.count = envs[k]->d.n; x.dev = envs[k]->cfg.device;
    f += x.count;
    s->sh.push_back(x);
  }
  if (int rc = finish_sharded(s)) { free_sharded(s); return rc; }
  *out = s;
  return GAQ_OK;
}

int gaq_destroy_sharded(gaq_sharded* s) {
  if (!s) return GAQ_OK;
  DeviceGuard guard;
  free_sharded(s);
  return GAQ_OK;
}

int gaq_sharded_num_shards(const gaq_sharded* s) { return s ? (int)s->sh.size() : GAQ_ERR_INVALID; }
int64_t gaq_sharded_num_envs(const gaq_sharded* s) { return s ? s->n : 0; }
gaq_env* gaq_sharded_shard(gaq_sharded* s, int32_t k) { return (s && k >= 0 && k < (int32_t)s->sh.size()) ? s->sh[k].env : nullptr; }
int gaq_sharded_range(const gaq_sharded* s, int32_t k, int64_t* first, int64_t* count, int32_t* device) {
  if (!s || k < 0 || k >= (int32_t)s->sh.size()) return fail(GAQ_ERR_INVALID, "sharded: no such shard");
  if (first) *first = s->sh[k].first;
  if (count) *count = s->sh[k].count;
  if (device) *device = s->sh[k].dev;
  return GAQ_OK;
}

int gaq_step_sharded_dev(gaq_sharded* s, const float* actions, float* obs, float* reward, uint8_t* done, void* stream) {
  if (!s || !actions || !obs || !reward || !done) return fail(GAQ_ERR_INVALID, "null argument");
  DeviceGuard guard;
  return fan_out(s, actions, nullptr, obs, reward, done, (hipStream_t)stream);
}

int gaq_reset_sharded_dev(gaq_sharded* s, const uint8_t* mask_dev, float* obs, void* stream) {
  if (!s || !obs) return fail(GAQ_ERR_INVALID, "null argument");
  DeviceGuard guard;
  return fan_out(s, nullptr, mask_dev, obs, nullptr, nullptr, (hipStream_t)stream);
}

int gaq_synchronize_sharded(gaq_sharded* s) {
  if (!s) return fail(GAQ_ERR_INVALID, "null handle");
  DeviceGuard guard;
  for (auto& x : s->sh) {
    HIP_TRY(hipSetDevice(x.dev));
    if (x.st) HIP_TRY(hipStreamSynchronize(x.st));
    if (int rc = sync_handle(x.env)) return rc;
  }
  HIP_TRY(hipSetDevice(s->root));
  HIP_TRY(hipStreamSynchronize(s->root_stream));
  return GAQ_OK;
}

int gaq_reset_sharded(gaq_sharded* s, const uint8_t* mask, float* obs_out) {
  if (!s || !obs_out) return fail(GAQ_ERR_INVALID, "null argument");
  DeviceGuard guard;
  if (int rc = gaq_synchronize_sharded(s)) return rc;
  if (int rc = need_stage(s)) return rc;
  const size_t n = (size_t)s->n, D = (size_t)s->D;
  HIP_TRY(hipSetDevice(s->root));
  if (mask) HIP_TRY(hipMemcpyAsync(s->stage + s->off_mask, mask, n, hipMemcpyHostToDevice, s->root_stream));
  if (int rc = fan_out(s, nullptr, mask ? reinterpret_cast<const uint8_t*>(s->stage + s->off_mask) : nullptr,
                       reinterpret_cast<float*>(s->stage + s->off_obs), nullptr, nullptr, s->root_stream)) return rc;
  HIP_TRY(hipSetDevice(s->root));
  HIP_TRY(hipMemcpyAsync(obs_out, s->stage + s->off_obs, 4 * D * n, hipMemcpyDeviceToHost, s->root_stream));
  HIP_TRY(hipStreamSynchronize(s->root_stream));
  return GAQ_OK;
}

int gaq_step_sharded(gaq_sharded* s, const float* actions, float* obs, float* reward, uint8_t* done) {
  if (!s || !actions || !obs || !reward || !done) return fail(GAQ_ERR_INVALID, "null argument");
  DeviceGuard guard;
  if (int rc = gaq_synchronize_sharded(s)) return rc;
  if (int rc = need_stage(s)) return rc;
  const size_t n = (size_t)s->n, D = (size_t)s->D;
  HIP_TRY(hipSetDevice(s->root));
  HIP_TRY(hipMemcpyAsync(s->stage, actions, 16 * n, hipMemcpyHostToDevice, s->root_stream));
  if (int rc = fan_out(s, reinterpret_cast<const float*>(s->stage), nullptr, reinterpret_cast<float*>(s->stage + s->off_obs),
                       reinterpret_cast<float*>(s->stage + s->off_rew), reinterpret_cast<uint8_t*>(s->stage + s->off_done), s->root_stream)) return rc;
  HIP_TRY(hipSetDevice(s->root));
  HIP_TRY(hipMemcpyAsync(obs, s->stage + s->off_obs, 4 * D * n, hipMemcpyDeviceToHost, s->root_stream));
  HIP_TRY(hipMemcpyAsync(reward, s->stage + s->off_rew, 4 * n, hipMemcpyDeviceToHost, s->root_stream));
  HIP_TRY(hipMemcpyAsync(done, s->stage + s->off_done, n, hipMemcpyDeviceToHost, s->root_stream));
  HIP_TRY(hipStreamSynchronize(s->root_stream));
  for (auto& x : s->sh) if (int rc = check_overrun(x.env)) return rc;
  // the reference raises on a non-finite reward inside step() (quadrotor.py:633-636)
  for (size_t i = 0; i < n; ++i) {
    if (!std::isfinite(reward[i])) {
      for (auto& x : s->sh) { HIP_TRY(hipSetDevice(x.dev)); HIP_TRY(hipMemset(x.env->d.nan_count, 0, sizeof(uint32_t))); }
      return fail(GAQ_ERR_NAN, "QuadEnv: reward is Nan");
    }
  }
  return GAQ_OK;
}

}  // extern "C"
