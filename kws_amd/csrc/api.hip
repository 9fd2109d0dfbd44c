// C ABI of libfastgrnn_hip.so (include/fastgrnn_hip.h): argument validation and
// dispatch between the MFMA-tiled fp32 scan and the generic scan.  Pure launches:
// no allocation, no synchronisation, no global state.
#include "common.h"

using namespace fastgrnn;

namespace {

bool nl_ok(int nl) { return nl >= FASTGRNN_NL_SIGMOID && nl <= FASTGRNN_NL_QUANT_SIGM4; }

int check_desc(const fastgrnn_desc* d) {
  if (!d) return FASTGRNN_ERR_NULL_POINTER;
  if (d->T < 1 || d->B < 1 || d->F < 1 || d->H < 1) return FASTGRNN_ERR_BAD_SHAPE;
  if (d->w_rank < 0 || d->u_rank < 0) return FASTGRNN_ERR_BAD_SHAPE;
  // every tensor is indexed with size_t inside the kernels; keep T*B*max(H,F) below 2^40
  if ((double)d->T * d->B * (d->H > d->F ? d->H : d->F) > 1099511627776.0) return FASTGRNN_ERR_BAD_SHAPE;
  if (!nl_ok(d->gate_nl) || !nl_ok(d->update_nl)) return FASTGRNN_ERR_BAD_NONLINEARITY;
  if (d->dtype != FASTGRNN_F32 && d->dtype != FASTGRNN_F64 && d->dtype != FASTGRNN_BF16_IO) return FASTGRNN_ERR_BAD_DTYPE;
  return FASTGRNN_OK;
}

int check_params(const fastgrnn_desc* d, const fastgrnn_params* p) {
  if (!p) return FASTGRNN_ERR_NULL_POINTER;
  if (d->w_rank ? (!p->w1 || !p->w2) : !p->w) return FASTGRNN_ERR_NULL_POINTER;
  if (d->u_rank ? (!p->u1 || !p->u2) : !p->u) return FASTGRNN_ERR_NULL_POINTER;
  if (!p->bias_gate || !p->bias_update || !p->zeta || !p->nu) return FASTGRNN_ERR_NULL_POINTER;
  return FASTGRNN_OK;
}

int check_ws(void* ws, size_t have, size_t need) {
  if (need == 0) return FASTGRNN_OK;
  if (!ws || have < need || (reinterpret_cast<uintptr_t>(ws) & 255u)) return FASTGRNN_ERR_WORKSPACE;
  return FASTGRNN_OK;
}

// 0 = generic scan, 1 = fp32-MFMA scan, 2 = split-precision scan on the bf16 matrix pipe
int pick_path(const fastgrnn_desc* d, int direction) {
  if (d->flags & FASTGRNN_FLAG_PREACT_AFFINE)        // the scaled forward: split-precision scans or the generic one
    return (!(d->flags & (FASTGRNN_FLAG_FORCE_GENERIC | FASTGRNN_FLAG_FORCE_F32_MFMA)) && affine_supported(*d)) ? 2 : 0;
  if (d->flags & FASTGRNN_FLAG_FORCE_GENERIC) return 0;
  if (!(d->flags & FASTGRNN_FLAG_FORCE_F32_MFMA) && split_supported(*d, direction)) return 2;
  return mfma_supported(*d, direction) ? 1 : 0;
}

size_t path_ws(const fastgrnn_desc& d, int path, int direction) {
  switch (path) {
    case 2: return direction ? split_backward_ws(d) : split_forward_ws(d);
    case 1: return direction ? mfma_backward_ws(d) : mfma_forward_ws(d);
    case 0: return direction ? generic_backward_ws(d) : generic_forward_ws(d);
    default: return 0;
  }
}

// What a caller's descriptor runs on and what that route needs from the caller.  resolve() validates and decides
// once; every entry point and every query starts from its answer and asks no predicate of its own.
struct route {
  fastgrnn_desc u;       // the descriptor without FASTGRNN_FLAG_ZERO_EXTEND / NO_INPUT_GRAD (which only sets
                         // plan.dx_optional): what a call runs on where the padded route does not apply
  fastgrnn_desc e;       // the padded descriptor, where plan.zext.forward
  int path[2];           // u's kernel family per direction; -1 where no unrolled call runs u in that direction
  size_t need[2];        // u's workspace per direction
  size_t zneed[2];       // the padded route's
  fastgrnn_plan plan;    // the public answers (fastgrnn_hip_plan); plan.zext.forward / backward: the padded route applies
};

// FASTGRNN_FLAG_ZERO_EXTEND (include/fastgrnn_hip.h): true when the forward takes the padded route, with r->e the padded
// descriptor; under FASTGRNN_FLAG_SAVE_PREACT the backward takes it too.  r->u and r->path are filled.
bool zext_route(const fastgrnn_desc* d, route* r) {
  if (!(d->flags & FASTGRNN_FLAG_ZERO_EXTEND)) return false;
  if (d->dtype != FASTGRNN_F32 && d->dtype != FASTGRNN_BF16_IO) return false;
  if (d->flags & (FASTGRNN_FLAG_FORCE_GENERIC | FASTGRNN_FLAG_FORCE_F32_MFMA | FASTGRNN_FLAG_X_BFT |
                  FASTGRNN_FLAG_PREACT_AFFINE | FASTGRNN_FLAG_BN_TRAIN))
    return false;
  if (d->H > 256 || d->F > 256) return false;
  const bool preact = (d->flags & FASTGRNN_FLAG_SAVE_PREACT) != 0;
  if (r->path[0] != 0 || (preact && r->path[1] != 0)) return false;
  const int Hp = d->H <= 128 ? 128 : 256;
  for (int Fp = 32; Fp <= 256; Fp *= 2) {
    if (Fp < d->F) continue;
    // element offsets of the padded copies are 32-bit (kernels_zext.hip)
    if ((double)d->T * d->B * (Hp > Fp ? Hp : Fp) >= 1073741824.0) return false;
    r->e = r->u;
    r->e.H = Hp;
    r->e.F = Fp;
    if (pick_path(&r->e, 0) == 2 && (!preact || pick_path(&r->e, 1) == 2)) return true;
  }
  return false;
}

int resolve(const fastgrnn_desc* d, route* r) {
  *r = route{};
  const int st = check_desc(d);
  if (st) return st;
  r->u = *d;
  r->u.flags &= ~(FASTGRNN_FLAG_ZERO_EXTEND | FASTGRNN_FLAG_NO_INPUT_GRAD);
  const fastgrnn_desc& u = r->u;
  const bool preact = (u.flags & FASTGRNN_FLAG_SAVE_PREACT) != 0;
  const bool affine = (u.flags & FASTGRNN_FLAG_PREACT_AFFINE) != 0;      // fastgrnn_hip_forward_unroll_affine: inference only
  const bool bn_train = (u.flags & FASTGRNN_FLAG_BN_TRAIN) != 0;         // fastgrnn_hip_bn_train_*
  for (int dir = 0; dir < 2; ++dir) {
    r->path[dir] = (bn_train || (affine && dir)) ? -1 : pick_path(&u, dir);
    if (r->path[dir] == 0 && !generic_lds_fits(u, dir)) r->path[dir] = -1;      // the floor itself has a limit: its LDS
    r->need[dir] = path_ws(u, r->path[dir], dir);
  }
  // d_x may be NULL (the input's gradient is not wanted) where it is a GEMM of its own behind the scan, and under
  // FASTGRNN_FLAG_NO_INPUT_GRAD where the scan can leave its d_x product out
  const bool nograd = (d->flags & FASTGRNN_FLAG_NO_INPUT_GRAD) != 0;
  const auto dx_optional = [nograd](const fastgrnn_desc& c) {
    const family* f = family_of(c);
    return (f && f->dx_optional) || (nograd && split_dx_skippable(c));
  };
  const family* fu = family_of(u);
  fastgrnn_plan& o = r->plan;
  fastgrnn_zext_plan& z = o.zext;
  if (zext_route(d, r)) {
    z.forward = 1;
    z.backward = preact;
    z.Hp = r->e.H;
    z.Fp = r->e.F;
    z.dx_optional = dx_optional(r->e);
    z.saved_bytes = zext_saved_bytes(*d, r->e);
    r->zneed[0] = zext_forward_ws(*d, r->e);
    if (preact) r->zneed[1] = zext_backward_ws(*d, r->e);
  }
  o.path[0] = z.forward ? 2 : r->path[0];
  o.path[1] = z.backward ? 2 : r->path[1];
  // forward workspace: under SAVE_PREACT every forward takes the padded route; without it a forward given the
  // (z_s, h_prime_s) pair runs as without the flag, so the answer covers that call as well
  o.workspace_bytes[0] = (z.forward && (preact || r->zneed[0] > r->need[0])) ? r->zneed[0] : r->need[0];
  o.workspace_bytes[1] = z.backward ? r->zneed[1] : r->need[1];
  // (path 2 only needs its workspace when no auxiliary output is requested: see split_forward_ws)
  o.forward_ws_optional = !affine && r->path[0] == 2 && fu && fu->forward_ws_optional;
  o.dx_optional = z.backward ? z.dx_optional : (r->path[1] == 2 && dx_optional(u));
  o.rank_space_cols = (preact && fu == &lowrank_family() && (r->path[0] == 2 || r->path[1] == 2)) ? 32 : 0;
  return FASTGRNN_OK;
}

// the gradient pointers a backward of d needs (fastgrnn_grads: the others are ignored)
int check_grads(const fastgrnn_desc& d, const fastgrnn_grads* g, bool dx_optional) {
  if ((!g->d_x && !dx_optional) || !g->d_bias_gate || !g->d_bias_update || !g->d_zeta || !g->d_nu || !g->d_h0)
    return FASTGRNN_ERR_NULL_POINTER;
  if (d.w_rank ? (!g->d_w1 || !g->d_w2) : !g->d_w) return FASTGRNN_ERR_NULL_POINTER;
  if (d.u_rank ? (!g->d_u1 || !g->d_u2) : !g->d_u) return FASTGRNN_ERR_NULL_POINTER;
  return FASTGRNN_OK;
}

// training-mode BatchNorm cell (FASTGRNN_FLAG_BN_TRAIN)
int check_bn_layer(const fastgrnn_bn_layer& l, bool forward) {
  if (!l.gamma || !l.beta) return FASTGRNN_ERR_NULL_POINTER;
  if (forward && (!l.running_mean || !l.running_var || (l.momentum < 0 && !l.num_batches_tracked)))
    return FASTGRNN_ERR_NULL_POINTER;
  if (!(l.eps >= 0) || !(l.momentum <= 1)) return FASTGRNN_ERR_BAD_SHAPE;
  return FASTGRNN_OK;
}

int check_bn_train(const fastgrnn_desc* d, const fastgrnn_params* p, const fastgrnn_bn_params* bn, bool forward) {
  int st;
  if (!(d->flags & FASTGRNN_FLAG_BN_TRAIN)) return FASTGRNN_ERR_UNSUPPORTED;
  if (d->B < 2) return FASTGRNN_ERR_BAD_SHAPE;                 // torch: more than 1 value per channel when training
  if ((st = check_params(d, p))) return st;
  if (!bn) return FASTGRNN_ERR_NULL_POINTER;
  const fastgrnn_bn_layer* layers[4] = {&bn->w, &bn->u, &bn->gate, &bn->update};
  for (const fastgrnn_bn_layer* l : layers)
    if ((st = check_bn_layer(*l, forward))) return st;
  if (!bn_train_supported(*d)) return FASTGRNN_ERR_UNSUPPORTED;
  return FASTGRNN_OK;
}

// fastgrnn_hip_forward_windows runs d on the windowed scans (flags outside the three it knows, FASTGRNN_FLAG_ZERO_EXTEND
// and NO_INPUT_GRAD among them, are refused: judged on d, not on r->u)
bool windows_route(const fastgrnn_desc* d, route* r) {
  return resolve(d, r) == FASTGRNN_OK && r->path[0] == 2 && windows_supported(*d);
}

// fastgrnn_hip_forward_windows_train / fastgrnn_hip_backward_windows run d (judged on d, as windows_route does: the two
// calls know FASTGRNN_FLAG_BATCH_MAJOR and, the backward, FASTGRNN_FLAG_GRAD_LAST; FASTGRNN_FLAG_SAVE_PREACT is theirs to
// add -- r->e is d with it -- and is refused like every other flag when the caller passes it)
bool train_windows_route(const fastgrnn_desc* d, route* r) {
  if (resolve(d, r) != FASTGRNN_OK || !train_windows_supported(*d)) return false;
  r->e = *d;
  r->e.flags |= FASTGRNN_FLAG_SAVE_PREACT;
  return true;
}

// the pool of a windowed training call: it holds a window, and its rows are addressed through the int32 starts (element
// offsets into the pool and its frame product are size_t: at most 2^31 rows of at most 256 floats cannot overflow them)
bool pool_rows_ok(const fastgrnn_desc* d, size_t pool_rows) {
  return pool_rows >= (size_t)d->T && pool_rows <= (size_t)INT32_MAX;
}

// r->u runs on the training kernels
bool bn_train_route(const fastgrnn_desc* d, route* r) {
  return resolve(d, r) == FASTGRNN_OK && (r->u.flags & FASTGRNN_FLAG_BN_TRAIN) && bn_train_supported(r->u);
}

const void* seg_state(const fastgrnn_update_seg& sg, int j) { return j == 0 ? sg.state0 : j == 1 ? sg.state1 : nullptr; }
const void* seg_state(const fastgrnn_optim_seg& sg, int j) { return sg.state[j]; }

// FASTGRNN_OK or the refusal of a segment array of either update call; needs: which of a segment's state slots 0..2
// the rule reads, as a bit mask
template <typename Seg>
int check_update_segs(const Seg* segs, int32_t n_segs, int needs, const int32_t* iht_mode) {
  for (int32_t k = 0; k < n_segs; ++k) {
    const Seg& sg = segs[k];
    if (!sg.param || !sg.grad) return FASTGRNN_ERR_NULL_POINTER;
    for (int j = 0; j < 3; ++j)
      if ((needs >> j & 1) && !seg_state(sg, j)) return FASTGRNN_ERR_NULL_POINTER;
    if (sg.iht && (!sg.support || !iht_mode)) return FASTGRNN_ERR_NULL_POINTER;
    if (sg.n < 1 || sg.n > FASTGRNN_UPDATE_MAX_N || sg.keep_rank < 0 || sg.keep_rank >= sg.n)
      return FASTGRNN_ERR_BAD_SHAPE;
  }
  return FASTGRNN_OK;
}
}  // namespace

extern "C" {

int fastgrnn_hip_abi_version(void) { return FASTGRNN_HIP_ABI_VERSION; }

const char* fastgrnn_hip_status_string(int status) {
  switch (status) {
    case FASTGRNN_OK: return "ok";
    case FASTGRNN_ERR_NULL_POINTER: return "a required pointer is NULL";
    case FASTGRNN_ERR_BAD_SHAPE: return "bad shape (T,B,F,H must be >= 1, ranks >= 0)";
    case FASTGRNN_ERR_BAD_NONLINEARITY: return "unknown nonlinearity code";
    case FASTGRNN_ERR_BAD_DTYPE: return "unsupported dtype";
    case FASTGRNN_ERR_WORKSPACE: return "workspace missing, too small or not 256-byte aligned";
    case FASTGRNN_ERR_LAUNCH: return "kernel launch failed";
    case FASTGRNN_ERR_UNSUPPORTED: return "configuration not supported";
    default: return "unknown status";
  }
}

int fastgrnn_hip_plan(const fastgrnn_desc* d, fastgrnn_plan* out) {
  if (!out) return FASTGRNN_ERR_NULL_POINTER;
  route r;
  const int st = resolve(d, &r);
  *out = r.plan;
  return st;
}

int fastgrnn_hip_kernel_path(const fastgrnn_desc* d, int direction) {
  route r;
  return resolve(d, &r) ? -1 : r.plan.path[direction ? 1 : 0];
}

size_t fastgrnn_hip_forward_workspace_bytes(const fastgrnn_desc* d) {
  route r;
  return resolve(d, &r) ? 0 : r.plan.workspace_bytes[0];
}

size_t fastgrnn_hip_backward_workspace_bytes(const fastgrnn_desc* d) {
  route r;
  return resolve(d, &r) ? 0 : r.plan.workspace_bytes[1];
}

int fastgrnn_hip_zero_extend_plan(const fastgrnn_desc* d, fastgrnn_zext_plan* out) {
  if (!out) return FASTGRNN_ERR_NULL_POINTER;
  route r;
  const int st = resolve(d, &r);
  *out = r.plan.zext;
  return st;
}

int fastgrnn_hip_forward_unroll(const fastgrnn_desc* dz, const fastgrnn_params* p, const void* x, const void* h0,
                                void* hs, void* z_s, void* c_s, void* workspace, size_t workspace_bytes,
                                void* stream) {
  route r;
  int st = resolve(dz, &r);
  if (st) return st;
  const fastgrnn_desc* d = &r.u;
  if ((st = check_params(d, p))) return st;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const bool preact = (d->flags & FASTGRNN_FLAG_SAVE_PREACT) != 0;
  if (r.plan.zext.forward && (preact || !z_s)) {      // (the reference's pair: as without the flag)
    if (!x || !h0 || !hs || (preact && !z_s)) return FASTGRNN_ERR_NULL_POINTER;
    if ((st = check_ws(workspace, workspace_bytes, r.zneed[0]))) return st;
    return zext_forward(*dz, r.e, *p, x, h0, hs, z_s, workspace, s);
  }
  if (!x || !h0 || !hs) return FASTGRNN_ERR_NULL_POINTER;
  if (d->flags & FASTGRNN_FLAG_PREACT_AFFINE) return FASTGRNN_ERR_UNSUPPORTED;   // fastgrnn_hip_forward_unroll_affine
  if (d->flags & FASTGRNN_FLAG_BN_TRAIN) return FASTGRNN_ERR_UNSUPPORTED;        // fastgrnn_hip_bn_train_forward
  if (r.path[0] < 0) return FASTGRNN_ERR_UNSUPPORTED;                            // no scan holds d in its LDS
  if (((d->flags & (FASTGRNN_FLAG_SAVE_PREACT | FASTGRNN_FLAG_BATCH_MAJOR | FASTGRNN_FLAG_X_BFT | FASTGRNN_FLAG_HS_LAST)) ||
       d->dtype == FASTGRNN_BF16_IO) && r.path[0] != 2)
    return FASTGRNN_ERR_UNSUPPORTED;
  if ((d->flags & FASTGRNN_FLAG_HS_LAST) && z_s) return FASTGRNN_ERR_UNSUPPORTED;   // nothing is saved for a backward
  if ((st = check_ws(workspace, workspace_bytes, (z_s && r.plan.forward_ws_optional) ? 0 : r.need[0]))) return st;
  switch (r.path[0]) {
    case 2: return split_forward(*d, *p, x, h0, hs, z_s, c_s, workspace, s);
    case 1: return mfma_forward(*d, *p, x, h0, hs, z_s, c_s, workspace, s);
    default: return generic_forward(*d, *p, x, h0, hs, z_s, c_s, workspace, s);
  }
}

int fastgrnn_hip_forward_unroll_affine(const fastgrnn_desc* dz, const fastgrnn_params* p, const void* gate_scale,
                                       const void* update_scale, const void* x, const void* h0, void* hs,
                                       void* workspace, size_t workspace_bytes, void* stream) {
  route r;
  int st = resolve(dz, &r);
  if (st) return st;
  const fastgrnn_desc* d = &r.u;
  if ((st = check_params(d, p))) return st;
  if (!gate_scale || !update_scale || !x || !h0 || !hs) return FASTGRNN_ERR_NULL_POINTER;
  if (!(d->flags & FASTGRNN_FLAG_PREACT_AFFINE) || d->dtype == FASTGRNN_BF16_IO || d->w_rank || d->u_rank ||
      (d->flags & (FASTGRNN_FLAG_SAVE_PREACT | FASTGRNN_FLAG_GRAD_LAST | FASTGRNN_FLAG_BN_TRAIN)))
    return FASTGRNN_ERR_UNSUPPORTED;
  if (r.path[0] < 0) return FASTGRNN_ERR_UNSUPPORTED;                            // no scan holds d in its LDS
  // (FASTGRNN_FLAG_X_BFT: path 2 takes it on the wide shapes -- affine_supported -- and nothing else does)
  if ((d->flags & (FASTGRNN_FLAG_BATCH_MAJOR | FASTGRNN_FLAG_HS_LAST | FASTGRNN_FLAG_X_BFT)) && r.path[0] != 2) return FASTGRNN_ERR_UNSUPPORTED;
  if ((st = check_ws(workspace, workspace_bytes, r.need[0]))) return st;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (r.path[0] == 2) return split_forward(*d, *p, x, h0, hs, nullptr, nullptr, workspace, s, gate_scale, update_scale);
  return generic_forward(*d, *p, x, h0, hs, nullptr, nullptr, workspace, s, gate_scale, update_scale);
}

int fastgrnn_hip_windows_supported(const fastgrnn_desc* d) {
  route r;
  return windows_route(d, &r) ? 1 : 0;
}

size_t fastgrnn_hip_forward_windows_workspace_bytes(const fastgrnn_desc* d, size_t pool_rows) {
  route r;
  if (!windows_route(d, &r) || pool_rows > (size_t)INT32_MAX) return 0;
  return windows_ws(*d, pool_rows);
}

int fastgrnn_hip_forward_windows(const fastgrnn_desc* d, const fastgrnn_params* p, const void* gate_scale,
                                 const void* update_scale, const void* x_pool, size_t pool_rows, const int32_t* x_start,
                                 const void* h0, void* hs, void* workspace, size_t workspace_bytes, void* stream) {
  route r;
  int st = resolve(d, &r);
  if (st) return st;
  if ((st = check_params(d, p))) return st;
  if (!x_pool || !x_start || !h0 || !hs) return FASTGRNN_ERR_NULL_POINTER;
  const bool affine = (d->flags & FASTGRNN_FLAG_PREACT_AFFINE) != 0;
  if ((gate_scale == nullptr) != (update_scale == nullptr) || (affine && !gate_scale)) return FASTGRNN_ERR_NULL_POINTER;
  if (gate_scale && !affine) return FASTGRNN_ERR_UNSUPPORTED;           // scales select the flag's arithmetic
  // rows are addressed through the int32 starts; element offsets into the pool and its frame product are size_t
  if (pool_rows < (size_t)d->T || pool_rows > (size_t)INT32_MAX ||
      (double)pool_rows * (d->H > d->F ? d->H : d->F) > 1099511627776.0)
    return FASTGRNN_ERR_BAD_SHAPE;
  if (r.path[0] != 2 || !windows_supported(*d)) return FASTGRNN_ERR_UNSUPPORTED;
  const size_t need = windows_ws(*d, pool_rows);
  if ((st = check_ws(workspace, workspace_bytes, need))) return st;
  const window_src win{x_start, pool_rows};
  return split_forward(*d, *p, x_pool, h0, hs, nullptr, nullptr, workspace, reinterpret_cast<hipStream_t>(stream),
                       gate_scale, update_scale, &win);
}

int fastgrnn_hip_train_windows_supported(const fastgrnn_desc* d) {
  route r;
  return train_windows_route(d, &r) ? 1 : 0;
}

size_t fastgrnn_hip_train_windows_forward_workspace_bytes(const fastgrnn_desc* d, size_t pool_rows) {
  route r;
  if (!train_windows_route(d, &r) || (d->flags & FASTGRNN_FLAG_GRAD_LAST) || pool_rows > (size_t)INT32_MAX) return 0;
  return train_windows_forward_ws(*d, pool_rows);
}

size_t fastgrnn_hip_train_windows_backward_workspace_bytes(const fastgrnn_desc* d, size_t pool_rows) {
  route r;
  if (!train_windows_route(d, &r) || pool_rows > (size_t)INT32_MAX) return 0;
  return train_windows_backward_ws(*d);
}

int fastgrnn_hip_forward_windows_train(const fastgrnn_desc* d, const fastgrnn_params* p, const void* x_pool,
                                       size_t pool_rows, const int32_t* x_start, const void* h0, void* hs, void* saved,
                                       void* workspace, size_t workspace_bytes, void* stream) {
  route r;
  int st = resolve(d, &r);
  if (st) return st;
  if ((st = check_params(d, p))) return st;
  if (!x_pool || !x_start || !h0 || !hs || !saved) return FASTGRNN_ERR_NULL_POINTER;
  if (!pool_rows_ok(d, pool_rows)) return FASTGRNN_ERR_BAD_SHAPE;
  if ((d->flags & FASTGRNN_FLAG_GRAD_LAST) || !train_windows_route(d, &r)) return FASTGRNN_ERR_UNSUPPORTED;
  if ((st = check_ws(workspace, workspace_bytes, train_windows_forward_ws(*d, pool_rows)))) return st;
  const window_src win{x_start, pool_rows};
  return split_forward(r.e, *p, x_pool, h0, hs, saved, nullptr, workspace, reinterpret_cast<hipStream_t>(stream),
                       nullptr, nullptr, &win);
}

int fastgrnn_hip_backward_windows(const fastgrnn_desc* d, const fastgrnn_params* p, const void* grad_hs,
                                  const void* x_pool, size_t pool_rows, const int32_t* x_start, const void* hs,
                                  const void* saved, const void* h0, const fastgrnn_grads* g, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  route r;
  int st = resolve(d, &r);
  if (st) return st;
  if ((st = check_params(d, p))) return st;
  if (!grad_hs || !x_pool || !x_start || !hs || !saved || !h0 || !g) return FASTGRNN_ERR_NULL_POINTER;
  if ((st = check_grads(*d, g, true))) return st;
  if (!pool_rows_ok(d, pool_rows)) return FASTGRNN_ERR_BAD_SHAPE;
  if (!train_windows_route(d, &r)) return FASTGRNN_ERR_UNSUPPORTED;
  if (g->d_x) return FASTGRNN_ERR_UNSUPPORTED;        // the pool's gradient is a scatter-add over the windows: not built
  if ((st = check_ws(workspace, workspace_bytes, train_windows_backward_ws(*d)))) return st;
  const window_src win{x_start, pool_rows};
  return split_backward(r.e, *p, grad_hs, x_pool, hs, saved, nullptr, h0, *g, workspace,
                        reinterpret_cast<hipStream_t>(stream), &win);
}

int fastgrnn_hip_backward_unroll(const fastgrnn_desc* dz, const fastgrnn_params* p, const void* grad_hs,
                                 const void* x, const void* hs, const void* z_s, const void* c_s, const void* h0,
                                 const fastgrnn_grads* g, void* workspace, size_t workspace_bytes, void* stream) {
  route r;
  int st = resolve(dz, &r);
  if (st) return st;
  const fastgrnn_desc* d = &r.u;
  if ((st = check_params(d, p))) return st;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (r.plan.zext.backward) {
    if (!grad_hs || !x || !hs || !z_s || !h0 || !g) return FASTGRNN_ERR_NULL_POINTER;
    if ((st = check_grads(*d, g, r.plan.dx_optional))) return st;
    if ((st = check_ws(workspace, workspace_bytes, r.zneed[1]))) return st;
    return zext_backward(*dz, r.e, *p, grad_hs, x, hs, z_s, h0, *g, workspace, s);
  }
  if (d->flags & FASTGRNN_FLAG_PREACT_AFFINE) return FASTGRNN_ERR_UNSUPPORTED;   // inference only
  if (d->flags & FASTGRNN_FLAG_BN_TRAIN) return FASTGRNN_ERR_UNSUPPORTED;        // fastgrnn_hip_bn_train_backward
  if (r.path[1] < 0) return FASTGRNN_ERR_UNSUPPORTED;                            // no scan holds d in its LDS
  const bool preact = (d->flags & FASTGRNN_FLAG_SAVE_PREACT) != 0;
  if ((preact || (d->flags & (FASTGRNN_FLAG_BATCH_MAJOR | FASTGRNN_FLAG_X_BFT | FASTGRNN_FLAG_GRAD_LAST)) || d->dtype == FASTGRNN_BF16_IO) && r.path[1] != 2)
    return FASTGRNN_ERR_UNSUPPORTED;
  if (!grad_hs || !x || !hs || !z_s || (!c_s && !preact) || !h0 || !g) return FASTGRNN_ERR_NULL_POINTER;
  if ((st = check_grads(*d, g, r.plan.dx_optional))) return st;
  if ((st = check_ws(workspace, workspace_bytes, r.need[1]))) return st;
  switch (r.path[1]) {
    case 2: return split_backward(*d, *p, grad_hs, x, hs, z_s, c_s, h0, *g, workspace, s);
    case 1: return mfma_backward(*d, *p, grad_hs, x, hs, z_s, c_s, h0, *g, workspace, s);
    default: return generic_backward(*d, *p, grad_hs, x, hs, z_s, c_s, h0, *g, workspace, s);
  }
}

// Single-step operators are the T = 1 case of the unrolled ones: hs[0] = new_h, and the
// backward's H_prev is old_h for t = 0 (hs itself is never read when T == 1).
int fastgrnn_hip_forward(const fastgrnn_desc* d, const fastgrnn_params* p, const void* x, const void* old_h,
                         void* new_h, void* z, void* c, void* workspace, size_t workspace_bytes, void* stream) {
  if (!d) return FASTGRNN_ERR_NULL_POINTER;
  if (d->T != 1) return FASTGRNN_ERR_BAD_SHAPE;
  return fastgrnn_hip_forward_unroll(d, p, x, old_h, new_h, z, c, workspace, workspace_bytes, stream);
}

int fastgrnn_hip_backward(const fastgrnn_desc* d, const fastgrnn_params* p, const void* grad_h, const void* x,
                          const void* old_h, const void* z, const void* c, const fastgrnn_grads* g,
                          void* workspace, size_t workspace_bytes, void* stream) {
  if (!d) return FASTGRNN_ERR_NULL_POINTER;
  if (d->T != 1) return FASTGRNN_ERR_BAD_SHAPE;
  fastgrnn_desc u = *d;
  u.flags &= ~FASTGRNN_FLAG_NO_INPUT_GRAD;           // ignored here: the single-step backward always writes d_x
  // hs is required non-NULL by the unrolled entry but never dereferenced at T == 1
  return fastgrnn_hip_backward_unroll(&u, p, grad_h, x, /*hs=*/old_h, z, c, old_h, g, workspace, workspace_bytes,
                                      stream);
}

size_t fastgrnn_hip_head_workspace_bytes(int32_t B, int32_t H, int32_t C) {
  return head_supported(B, H, C) ? head_ws_bytes(B, H, C) : 0;
}

int fastgrnn_hip_head_xent(int32_t B, int32_t H, int32_t C, const void* h_last, const void* fc_w, const void* fc_b,
                           const int64_t* labels, void* loss, void* log_probs, void* d_h_last, void* d_fc_w,
                           void* d_fc_b, void* workspace, size_t workspace_bytes, void* stream) {
  if (B < 1 || H < 1 || C < 1) return FASTGRNN_ERR_BAD_SHAPE;
  if (!head_supported(B, H, C)) return FASTGRNN_ERR_UNSUPPORTED;
  if (!h_last || !fc_w || !fc_b || !labels || !loss || !d_h_last || !d_fc_w || !d_fc_b) return FASTGRNN_ERR_NULL_POINTER;
  int st = check_ws(workspace, workspace_bytes, head_ws_bytes(B, H, C));
  if (st) return st;
  return head_xent(B, H, C, h_last, fc_w, fc_b, labels, loss, log_probs, d_h_last, d_fc_w, d_fc_b, workspace,
                   reinterpret_cast<hipStream_t>(stream));
}

size_t fastgrnn_hip_head_predict_workspace_bytes(int32_t B, int32_t H, int32_t C) {
  return head_supported(B, H, C) ? head_predict_ws_bytes(B) : 0;
}

int fastgrnn_hip_head_predict(int32_t B, int32_t H, int32_t C, const void* h_last, const void* fc_w, const void* fc_b,
                              const int64_t* labels, void* log_probs, int32_t* pred, int32_t* n_correct,
                              void* workspace, size_t workspace_bytes, void* stream) {
  if (B < 1 || H < 1 || C < 1) return FASTGRNN_ERR_BAD_SHAPE;
  if (!head_supported(B, H, C)) return FASTGRNN_ERR_UNSUPPORTED;
  if (!h_last || !fc_w || !fc_b || !pred || (labels && !n_correct)) return FASTGRNN_ERR_NULL_POINTER;
  int st = check_ws(workspace, workspace_bytes, labels ? head_predict_ws_bytes(B) : 0);   // (only the count uses it)
  if (st) return st;
  return head_predict(B, H, C, h_last, fc_w, fc_b, labels, log_probs, pred, n_correct, workspace,
                      reinterpret_cast<hipStream_t>(stream));
}

int fastgrnn_hip_vote_windows(int32_t S, int32_t Nw, int32_t num_windows, int32_t majority, const int32_t* pred,
                              int32_t* majority_out, int32_t* event_out, void* stream) {
  if (S < 1 || Nw < 1 || num_windows < 1 || majority < 1 || majority > num_windows) return FASTGRNN_ERR_BAD_SHAPE;
  if ((double)S * Nw > 1099511627776.0) return FASTGRNN_ERR_BAD_SHAPE;     // (element offsets are size_t; as check_desc)
  if (!vote_supported(num_windows)) return FASTGRNN_ERR_UNSUPPORTED;
  if (!pred || !majority_out || !event_out) return FASTGRNN_ERR_NULL_POINTER;
  return vote_windows(S, Nw, num_windows, majority, pred, majority_out, event_out, reinterpret_cast<hipStream_t>(stream));
}

// FASTGRNN_OK or the refusal of train_update's arguments; count: the step scalar, or the guard state that replaces it
static int check_train_update(const fastgrnn_update_hyper* h, const fastgrnn_update_seg* segs, int32_t n_segs,
                              const float* lr, const void* count, const int32_t* iht_mode) {
  if (!h || !segs || !lr || !count) return FASTGRNN_ERR_NULL_POINTER;
  if (h->algo != 0 && h->algo != 1) return FASTGRNN_ERR_UNSUPPORTED;
  if (n_segs < 1) return FASTGRNN_ERR_BAD_SHAPE;
  const bool adam = h->algo == 0;
  const double b1 = h->beta1_or_momentum, b2 = h->beta2_or_dampening;
  // (written so that a NaN fails every range check)
  if (!(b1 >= 0.0 && b1 < 1.0) || !(h->weight_decay >= 0.0)) return FASTGRNN_ERR_BAD_SHAPE;
  if (adam && (!(b2 >= 0.0 && b2 < 1.0) || !(h->eps > 0.0))) return FASTGRNN_ERR_BAD_SHAPE;
  if (!adam && h->nesterov && (b1 <= 0.0 || b2 != 0.0)) return FASTGRNN_ERR_BAD_SHAPE;   // torch.optim.SGD's rule
  if (!adam && !(b2 == b2)) return FASTGRNN_ERR_BAD_SHAPE;
  return check_update_segs(segs, n_segs, adam ? 3 : 1, iht_mode);
}

int fastgrnn_hip_train_update(const fastgrnn_update_hyper* h, const fastgrnn_update_seg* segs, int32_t n_segs,
                              const float* lr, const int64_t* step, const int32_t* iht_mode, void* stream) {
  if (const int st = check_train_update(h, segs, n_segs, lr, step, iht_mode)) return st;
  return update_step(*h, segs, n_segs, lr, step, iht_mode, nullptr, reinterpret_cast<hipStream_t>(stream));
}

// ... and of optim_update's
static int check_optim_update(const fastgrnn_optim_hyper* h, const fastgrnn_optim_seg* segs, int32_t n_segs,
                              const float* lr, const void* count, const int32_t* iht_mode, const float* scalars) {
  if (!h || !segs || !lr || !count) return FASTGRNN_ERR_NULL_POINTER;
  if (h->algo < 2 || h->algo > 7) return FASTGRNN_ERR_UNSUPPORTED;
  if (n_segs < 1) return FASTGRNN_ERR_BAD_SHAPE;
  const double* v = h->h;
  bool ok = false;                    // (every comparison written so that a NaN fails it)
  int needs = 1;                      // which of state[0..2] the rule reads, as a bit mask
  switch (h->algo) {
    case 2:                           // RMSprop: alpha, eps, momentum
      ok = v[0] >= 0.0 && v[1] > 0.0 && v[2] >= 0.0 && h->weight_decay >= 0.0;
      needs = 1 | (v[2] > 0.0 ? 2 : 0) | ((h->flags & 1) ? 4 : 0);
      break;
    case 3:                           // Adagrad: lr_decay, eps
      ok = v[0] >= 0.0 && v[1] > 0.0 && h->weight_decay >= 0.0;
      break;
    case 4:                           // Adadelta: rho, eps
      ok = v[0] >= 0.0 && v[0] <= 1.0 && v[1] > 0.0 && h->weight_decay >= 0.0;
      needs = 3;
      break;
    case 5:                           // Adamax: beta1, beta2, eps
      ok = v[0] >= 0.0 && v[0] < 1.0 && v[1] >= 0.0 && v[1] < 1.0 && v[2] > 0.0 && h->weight_decay >= 0.0;
      needs = 3;
      break;
    case 6:                           // ASGD: lambd, alpha, t0 (torch takes any value)
      ok = v[0] == v[0] && v[1] == v[1] && v[2] == v[2] && h->weight_decay >= 0.0;
      if (!scalars) return FASTGRNN_ERR_NULL_POINTER;
      break;
    default:                          // Rprop: etaminus, etaplus, step_min, step_max
      ok = v[0] > 0.0 && v[0] < 1.0 && v[1] > 1.0 && v[2] <= v[3] && h->weight_decay == 0.0;
      needs = 3;
      break;
  }
  if (!ok) return FASTGRNN_ERR_BAD_SHAPE;
  return check_update_segs(segs, n_segs, needs, iht_mode);
}

int fastgrnn_hip_optim_update(const fastgrnn_optim_hyper* h, const fastgrnn_optim_seg* segs, int32_t n_segs,
                              const float* lr, const int64_t* step, const int32_t* iht_mode, float* scalars,
                              void* stream) {
  if (const int st = check_optim_update(h, segs, n_segs, lr, step, iht_mode, scalars)) return st;
  return update_step(*h, segs, n_segs, lr, step, iht_mode, scalars, reinterpret_cast<hipStream_t>(stream));
}

size_t fastgrnn_hip_grad_guard_workspace_bytes(int32_t n_segs) { return grad_guard_ws_bytes(n_segs); }

int fastgrnn_hip_grad_guard(const fastgrnn_guard_seg* segs, int32_t n_segs, double max_norm, int32_t flags,
                            fastgrnn_guard_state* state, void* workspace, size_t workspace_bytes, void* stream) {
  if (!segs || !state || !workspace) return FASTGRNN_ERR_NULL_POINTER;
  if (n_segs < 1 || !(max_norm > 0.0)) return FASTGRNN_ERR_BAD_SHAPE;          // (a NaN max_norm fails the comparison)
  if (flags & ~FASTGRNN_GUARD_SKIP_NONFINITE) return FASTGRNN_ERR_UNSUPPORTED;
  for (int32_t k = 0; k < n_segs; ++k) {
    if (!segs[k].grad) return FASTGRNN_ERR_NULL_POINTER;
    if (segs[k].n < 1 || segs[k].n > FASTGRNN_UPDATE_MAX_N) return FASTGRNN_ERR_BAD_SHAPE;
  }
  if (workspace_bytes < grad_guard_ws_bytes(n_segs) || (reinterpret_cast<uintptr_t>(workspace) & 7))
    return FASTGRNN_ERR_WORKSPACE;
  return grad_guard_run(segs, n_segs, max_norm, flags, state, workspace, reinterpret_cast<hipStream_t>(stream));
}

int fastgrnn_hip_train_update_guarded(const fastgrnn_update_hyper* h, const fastgrnn_update_seg* segs, int32_t n_segs,
                                      const float* lr, const fastgrnn_guard_state* guard, const int32_t* iht_mode,
                                      void* stream) {
  if (const int st = check_train_update(h, segs, n_segs, lr, guard, iht_mode)) return st;
  return update_step_guarded(*h, segs, n_segs, lr, guard, iht_mode, nullptr, reinterpret_cast<hipStream_t>(stream));
}

int fastgrnn_hip_optim_update_guarded(const fastgrnn_optim_hyper* h, const fastgrnn_optim_seg* segs, int32_t n_segs,
                                      const float* lr, const fastgrnn_guard_state* guard, const int32_t* iht_mode,
                                      float* scalars, void* stream) {
  if (const int st = check_optim_update(h, segs, n_segs, lr, guard, iht_mode, scalars)) return st;
  return update_step_guarded(*h, segs, n_segs, lr, guard, iht_mode, scalars, reinterpret_cast<hipStream_t>(stream));
}

// FASTGRNN_OK or the refusal of a featuriser descriptor (include/fastgrnn_hip.h lists the supported range)
static int check_mfcc_desc(const fastgrnn_mfcc_desc* d) {
  if (!d) return FASTGRNN_ERR_NULL_POINTER;
  if (d->B < 1 || d->L < 1 || d->clip_stride < 1 || d->max_len < 1 || d->n_mfcc < 1) return FASTGRNN_ERR_BAD_SHAPE;
  if (!(d->top_db == d->top_db)) return FASTGRNN_ERR_BAD_SHAPE;
  if (d->audio_dtype != FASTGRNN_MFCC_AUDIO_F32 && d->audio_dtype != FASTGRNN_MFCC_AUDIO_I16) return FASTGRNN_ERR_BAD_DTYPE;
  if (d->L < 1280 || d->L > 16000 || d->n_mfcc > 64 || d->order < 0 || d->order > 2) return FASTGRNN_ERR_UNSUPPORTED;
  if (d->width < 3 || d->width > 15 || !(d->width & 1) || d->L < 160 * (d->width - 1)) return FASTGRNN_ERR_UNSUPPORTED;
  if (d->flags & ~(uint32_t)FASTGRNN_MFCC_PEAK_NORMALIZE) return FASTGRNN_ERR_UNSUPPORTED;
  // (element offsets are size_t and the workgroup's block of the output is indexed in 32 bits)
  const double per_clip = (double)d->max_len * d->n_mfcc * (d->order + 1);
  if (per_clip > 1073741824.0 || per_clip * d->B > 1099511627776.0) return FASTGRNN_ERR_BAD_SHAPE;
  return FASTGRNN_OK;
}

size_t fastgrnn_hip_mfcc_tables_bytes(void) { return mfcc_tables_bytes(); }

int fastgrnn_hip_mfcc_init_tables(void* tables, void* stream) {
  if (!tables) return FASTGRNN_ERR_NULL_POINTER;
  return mfcc_init_tables(tables, reinterpret_cast<hipStream_t>(stream));
}

size_t fastgrnn_hip_mfcc_workspace_bytes(const fastgrnn_mfcc_desc* d) {
  (void)d;
  return 0;                                      // (everything between the samples and the rows stays in LDS)
}

int fastgrnn_hip_mfcc(const fastgrnn_mfcc_desc* d, const void* audio, const int32_t* lengths, const void* tables,
                      const float* mean, const float* std, void* feats, void* workspace, size_t workspace_bytes,
                      void* stream) {
  int st = check_mfcc_desc(d);
  if (st) return st;
  if (!audio || !tables || !feats || (!mean != !std)) return FASTGRNN_ERR_NULL_POINTER;
  if ((st = check_ws(workspace, workspace_bytes, fastgrnn_hip_mfcc_workspace_bytes(d)))) return st;
  return mfcc_run(*d, audio, lengths, tables, mean, std, feats, reinterpret_cast<hipStream_t>(stream));
}

// FASTGRNN_OK or the refusal of what the streamed featuriser reads of the recording itself: all the frames call reads
static int check_stream_recording(const fastgrnn_mfcc_stream_desc* d) {
  if (!d) return FASTGRNN_ERR_NULL_POINTER;
  if (d->N < 1 || d->hop < 1) return FASTGRNN_ERR_BAD_SHAPE;
  if (d->audio_dtype != FASTGRNN_MFCC_AUDIO_F32 && d->audio_dtype != FASTGRNN_MFCC_AUDIO_I16) return FASTGRNN_ERR_BAD_DTYPE;
  if (d->hop % 160 || d->N < 16000 || d->N >= 2147483648ll) return FASTGRNN_ERR_UNSUPPORTED;
  return FASTGRNN_OK;
}

// ... and of the clips and the feature settings: a clip of the streamed call is a clip of fastgrnn_hip_mfcc with
// L = 16000 and clip_stride = hop, so the settings go through that call's own check
static int check_stream_clips(const fastgrnn_mfcc_stream_desc* d) {
  if (!d) return FASTGRNN_ERR_NULL_POINTER;
  if (d->N < 1 || d->hop < 1 || d->B < 1 || d->clip0 < 0) return FASTGRNN_ERR_BAD_SHAPE;
  fastgrnn_mfcc_desc m;
  m.B = d->B;
  m.L = 16000;
  m.clip_stride = d->hop;
  m.audio_dtype = d->audio_dtype;
  m.n_mfcc = d->n_mfcc;
  m.order = d->order;
  m.width = d->width;
  m.max_len = d->max_len;
  m.top_db = d->top_db;
  m.flags = d->flags;
  int st = check_mfcc_desc(&m);
  if (st == FASTGRNN_ERR_BAD_SHAPE || st == FASTGRNN_ERR_BAD_DTYPE) return st;
  const int rec = check_stream_recording(d);
  if (rec) return rec;
  if (st) return st;
  if ((int64_t)d->clip0 + d->B > (d->N - 16000) / d->hop + 1) return FASTGRNN_ERR_BAD_SHAPE;
  return FASTGRNN_OK;
}

size_t fastgrnn_hip_mfcc_stream_workspace_bytes(const fastgrnn_mfcc_stream_desc* d) {
  return check_stream_recording(d) ? 0 : mfcc_stream_ws_bytes(*d);
}

// (a NULL workspace is refused before this as a missing operand: the two calls exist to share one)
static int check_stream_ws(const fastgrnn_mfcc_stream_desc* d, void* workspace, size_t workspace_bytes) {
  if (workspace_bytes < mfcc_stream_ws_bytes(*d) || (reinterpret_cast<uintptr_t>(workspace) & 255u))
    return FASTGRNN_ERR_WORKSPACE;
  return FASTGRNN_OK;
}

int fastgrnn_hip_mfcc_stream_frames(const fastgrnn_mfcc_stream_desc* d, const void* audio, const void* tables,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  int st = check_stream_recording(d);
  if (st) return st;
  if (!audio || !tables || !workspace) return FASTGRNN_ERR_NULL_POINTER;
  if ((st = check_stream_ws(d, workspace, workspace_bytes))) return st;
  return mfcc_stream_frames_run(*d, audio, tables, workspace, reinterpret_cast<hipStream_t>(stream));
}

int fastgrnn_hip_mfcc_stream_clips(const fastgrnn_mfcc_stream_desc* d, const void* audio, const void* tables,
                                   void* workspace, size_t workspace_bytes, const float* mean, const float* std,
                                   void* feats, void* stream) {
  int st = check_stream_clips(d);
  if (st) return st;
  if (!audio || !tables || !workspace || !feats || (!mean != !std)) return FASTGRNN_ERR_NULL_POINTER;
  if ((st = check_stream_ws(d, workspace, workspace_bytes))) return st;
  return mfcc_stream_clips_run(*d, audio, tables, workspace, mean, std, feats, reinterpret_cast<hipStream_t>(stream));
}

// the noise bank's sizes, as both augmentation calls read them
static int check_noise_bank(int32_t n_noise, int32_t noise_len_max, const int32_t* noise_lengths) {
  if (n_noise < 0) return FASTGRNN_ERR_BAD_SHAPE;
  if (n_noise > 0 && !noise_lengths) return FASTGRNN_ERR_NULL_POINTER;
  if (n_noise > 0 && (noise_len_max < 1 || noise_len_max > FASTGRNN_MFCC_NOISE_LEN_MAX)) return FASTGRNN_ERR_UNSUPPORTED;
  return FASTGRNN_OK;
}

int fastgrnn_hip_mfcc_augment(const fastgrnn_mfcc_desc* d, const fastgrnn_mfcc_bank* bank, const void* audio,
                              const int32_t* lengths, const void* noise, const int32_t* noise_lengths,
                              const fastgrnn_mfcc_aug* aug, const void* tables, const float* mean, const float* std,
                              void* feats, void* workspace, size_t workspace_bytes, void* stream) {
  int st = check_mfcc_desc(d);
  if (st) return st;
  if (!bank || !aug || !audio || !tables || !feats || (!mean != !std)) return FASTGRNN_ERR_NULL_POINTER;
  if (bank->n_clips < 1 || bank->n_noise < 0 || (bank->n_noise > 0 && bank->noise_stride < 1)) return FASTGRNN_ERR_BAD_SHAPE;
  if (bank->n_noise > 0 && !noise) return FASTGRNN_ERR_NULL_POINTER;
  if ((st = check_noise_bank(bank->n_noise, bank->noise_len_max, noise_lengths))) return st;
  if ((st = check_ws(workspace, workspace_bytes, fastgrnn_hip_mfcc_workspace_bytes(d)))) return st;
  return mfcc_augment_run(*d, *bank, audio, lengths, noise, noise_lengths, aug, tables, mean, std, feats,
                          reinterpret_cast<hipStream_t>(stream));
}

int fastgrnn_hip_augment_draw(int32_t B, uint64_t seed, const int64_t* step, const int32_t* index,
                              const fastgrnn_augment_ranges* r, int32_t n_noise, int32_t noise_len_max,
                              const int32_t* noise_lengths, fastgrnn_mfcc_aug* aug, void* stream) {
  if (!r || !step || !index || !aug) return FASTGRNN_ERR_NULL_POINTER;
  if (B < 1) return FASTGRNN_ERR_BAD_SHAPE;
  int st = check_noise_bank(n_noise, noise_len_max, noise_lengths);
  if (st) return st;
  // (written so that a NaN fails every range check; lo <= hi, both and their difference finite)
  if (!(r->p_augment >= 0.f && r->p_augment <= 1.f) || !(r->p_noise >= 0.f && r->p_noise <= 1.f)) return FASTGRNN_ERR_BAD_SHAPE;
  const float inf = __builtin_huge_valf();
  if (!(r->gain_lo <= r->gain_hi && r->gain_lo > -inf && r->gain_hi - r->gain_lo < inf)) return FASTGRNN_ERR_BAD_SHAPE;
  if (!(r->noise_gain_lo <= r->noise_gain_hi && r->noise_gain_lo > -inf && r->noise_gain_hi - r->noise_gain_lo < inf)) return FASTGRNN_ERR_BAD_SHAPE;
  if (r->max_shift < 0 || r->max_shift > FASTGRNN_AUGMENT_MAX_SHIFT) return FASTGRNN_ERR_UNSUPPORTED;
  return augment_draw_run(B, seed, step, index, *r, n_noise, noise_len_max, noise_lengths, aug,
                          reinterpret_cast<hipStream_t>(stream));
}

// the refusals of a schedule descriptor, in train_schedule's order
static int check_schedule_desc(const fastgrnn_schedule_desc* d) {
  if (!d) return FASTGRNN_ERR_NULL_POINTER;
  if (d->B < 1 || d->world < 1 || d->rank < 0 || d->rank >= d->world) return FASTGRNN_ERR_BAD_SHAPE;
  const int64_t per_tick = (int64_t)d->B * d->world;
  if (per_tick > INT32_MAX || d->N < per_tick) return FASTGRNN_ERR_BAD_SHAPE;
  if (d->num_epochs < 1 || d->trim_level < 1 || d->log_len < 1) return FASTGRNN_ERR_BAD_SHAPE;
  if (d->lr_lead != 0 && d->lr_lead != 1) return FASTGRNN_ERR_BAD_SHAPE;
  if (d->lr_kind < FASTGRNN_LR_CONSTANT || d->lr_kind > FASTGRNN_LR_EXPONENTIAL_RESETTING) return FASTGRNN_ERR_UNSUPPORTED;
  // (written so that a NaN fails every range check)
  const double inf = __builtin_huge_val();
  if (!(d->lr_base >= 0.0 && d->lr_base < inf) || !(d->lr_min >= 0.0 && d->lr_min < inf)) return FASTGRNN_ERR_BAD_SHAPE;
  const int kind = d->lr_kind;
  if (kind != FASTGRNN_LR_CONSTANT && kind != FASTGRNN_LR_COSINE && !(d->gamma > 0.0 && d->gamma < inf))
    return FASTGRNN_ERR_BAD_SHAPE;
  if (kind == FASTGRNN_LR_TRIANGLE && !(d->stepsize > 0.0 && d->stepsize < inf)) return FASTGRNN_ERR_BAD_SHAPE;
  if (kind == FASTGRNN_LR_COSINE && !(d->t_max > 0.0 && d->t_max < inf)) return FASTGRNN_ERR_BAD_SHAPE;
  if (kind == FASTGRNN_LR_STEP && d->step_size < 1) return FASTGRNN_ERR_BAD_SHAPE;
  if (kind == FASTGRNN_LR_EXPONENTIAL_RESETTING && d->reset < 0) return FASTGRNN_ERR_BAD_SHAPE;
  return FASTGRNN_OK;
}

int fastgrnn_hip_train_schedule(const fastgrnn_schedule_desc* d, const int64_t* step, int32_t* index, float* lr,
                                int32_t* iht_mode, int64_t* where, void* stream) {
  const int st = check_schedule_desc(d);
  if (st) return st;
  if (!step || !index || !lr || !where || (d->sparsify && !iht_mode)) return FASTGRNN_ERR_NULL_POINTER;
  return train_schedule_run(*d, step, index, lr, iht_mode, where, reinterpret_cast<hipStream_t>(stream));
}

// what both rolling calls refuse of the pair of descriptors (d has passed check_schedule_desc)
static int check_rolling_desc(const fastgrnn_schedule_desc* d, const fastgrnn_rolling_desc* r) {
  if (d->N / (d->B * d->world) < 2) return FASTGRNN_ERR_BAD_SHAPE;
  if (r->max_rolling_length < 0 || r->bag_count < 1) return FASTGRNN_ERR_BAD_SHAPE;
  if ((int64_t)d->B * r->bag_count > INT32_MAX) return FASTGRNN_ERR_BAD_SHAPE;
  return FASTGRNN_OK;
}

int fastgrnn_hip_train_schedule_rolling(const fastgrnn_schedule_desc* d, const fastgrnn_rolling_desc* r,
                                        const int64_t* step, int32_t* index, float* lr, int32_t* iht_mode,
                                        int64_t* where, void* stream) {
  if (!d || !r) return FASTGRNN_ERR_NULL_POINTER;
  int st = check_schedule_desc(d);
  if (st || (st = check_rolling_desc(d, r))) return st;
  if (!step || !index || !lr || !where || (d->sparsify && !iht_mode)) return FASTGRNN_ERR_NULL_POINTER;
  return train_schedule_rolling_run(*d, *r, step, index, lr, iht_mode, where, reinterpret_cast<hipStream_t>(stream));
}

int fastgrnn_hip_rolling_exchange(const fastgrnn_schedule_desc* d, const fastgrnn_rolling_desc* r, const int64_t* step,
                                  const float* const state[3], float* const bag[3], float* const h0[3], void* stream) {
  if (!d || !r) return FASTGRNN_ERR_NULL_POINTER;
  int st = check_schedule_desc(d);
  if (st || (st = check_rolling_desc(d, r))) return st;
  if (r->layers < 1 || r->layers > 3) return FASTGRNN_ERR_BAD_SHAPE;
  for (int l = 0; l < r->layers; ++l)
    if (r->H[l] < 1) return FASTGRNN_ERR_BAD_SHAPE;
  if (!step || !state || !bag || !h0) return FASTGRNN_ERR_NULL_POINTER;
  for (int l = 0; l < r->layers; ++l)
    if (!state[l] || !bag[l] || !h0[l]) return FASTGRNN_ERR_NULL_POINTER;
  return rolling_exchange_run(*d, *r, step, state, bag, h0, reinterpret_cast<hipStream_t>(stream));
}

int fastgrnn_hip_frame_gemm(size_t rows, int32_t H, int32_t F, const void* x, const void* w, void* p, int32_t dtype,
                            void* stream) {
  if (!x || !w || !p) return FASTGRNN_ERR_NULL_POINTER;
  if (rows < 1 || H < 1 || F < 1) return FASTGRNN_ERR_BAD_SHAPE;
  if (dtype != FASTGRNN_F32 && dtype != FASTGRNN_BF16_IO) return FASTGRNN_ERR_BAD_DTYPE;
  if (!rows_gemm_supported(H, F, false)) return FASTGRNN_ERR_UNSUPPORTED;
  return rows_gemm(rows, H, F, false, x, reinterpret_cast<const float*>(w), p, dtype == FASTGRNN_BF16_IO, false,
                   reinterpret_cast<hipStream_t>(stream));
}

int fastgrnn_hip_bn_train_supported(const fastgrnn_desc* d) {
  route r;
  return bn_train_route(d, &r) ? 1 : 0;
}

size_t fastgrnn_hip_bn_train_forward_workspace_bytes(const fastgrnn_desc* d) {
  route r;
  return bn_train_route(d, &r) ? bn_train_forward_ws(r.u) : 0;
}

size_t fastgrnn_hip_bn_train_backward_workspace_bytes(const fastgrnn_desc* d) {
  route r;
  return bn_train_route(d, &r) ? bn_train_backward_ws(r.u) : 0;
}

int fastgrnn_hip_bn_train_forward(const fastgrnn_desc* dz, const fastgrnn_params* p, const fastgrnn_bn_params* bn,
                                  const void* x, const void* h0, void* hs, void* saved, void* stats, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  route r;
  int st = resolve(dz, &r);
  if (st) return st;
  const fastgrnn_desc* d = &r.u;
  if ((st = check_bn_train(d, p, bn, true))) return st;
  if (!x || !h0 || !hs || !saved || !stats) return FASTGRNN_ERR_NULL_POINTER;
  if ((st = check_ws(workspace, workspace_bytes, bn_train_forward_ws(*d)))) return st;
  return bn_train_forward(*d, *p, *bn, x, h0, hs, saved, stats, workspace, reinterpret_cast<hipStream_t>(stream));
}

int fastgrnn_hip_bn_train_backward(const fastgrnn_desc* dz, const fastgrnn_params* p, const fastgrnn_bn_params* bn,
                                   const void* grad_hs, const void* x, const void* hs, const void* saved,
                                   const void* stats, const void* h0, const fastgrnn_grads* g,
                                   const fastgrnn_bn_grads* bg, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  route r;
  int st = resolve(dz, &r);
  if (st) return st;
  const fastgrnn_desc* d = &r.u;
  if ((st = check_bn_train(d, p, bn, false))) return st;
  if (!grad_hs || !x || !hs || !saved || !stats || !h0 || !g || !bg) return FASTGRNN_ERR_NULL_POINTER;
  if (!g->d_h0 || !g->d_w || !g->d_u || !g->d_bias_gate || !g->d_bias_update || !g->d_zeta || !g->d_nu)
    return FASTGRNN_ERR_NULL_POINTER;
  if (!bg->d_gamma_w || !bg->d_beta_w || !bg->d_gamma_u || !bg->d_beta_u || !bg->d_gamma_gate || !bg->d_beta_gate ||
      !bg->d_gamma_update || !bg->d_beta_update)
    return FASTGRNN_ERR_NULL_POINTER;
  if ((st = check_ws(workspace, workspace_bytes, bn_train_backward_ws(*d)))) return st;
  return bn_train_backward(*d, *p, *bn, grad_hs, x, hs, saved, stats, h0, *g, *bg, workspace,
                           reinterpret_cast<hipStream_t>(stream));
}

int fastgrnn_hip_debug_poison_cu_state(uint32_t pattern, void* stream) {
  return debug_poison(pattern, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
