// Hidden sizes up to 256 on the split-precision scans by zero-extension (FASTGRNN_FLAG_ZERO_EXTEND).
// A cell of hidden size H <= 256 and input size F that would run on the generic scan is run as the cell of the padded
// shape (Hp, Fp) that kernel path 2 covers: W, U (or the factors), the two biases, h0, x and grad_hs are copied into
// zero-filled padded buffers, the existing path-2 code runs on them unchanged, and hs, d_x, d_h0 and the parameter
// gradients are compacted back.  A padded unit has pre-activation 0 at every step: its rows of W, U and the biases
// are zero, so its candidate tanh(0) = 0 and, with h0 = 0 there, its state stays 0; its columns of U are zero, so it
// never feeds a real unit, and every gradient it contributes is an exact zero.  The real units therefore get exactly
// what the library computes for the explicitly padded problem.
//
// The copies are plain bandwidth-bound kernels: no LDS, no MFMA, no inline assembly, no allocation or synchronisation
// (graph-capturable on the caller's stream).  One launch takes up to ZJ copies (a 2-D grid, y = the copy).
#include "common.h"

namespace fastgrnn {
namespace {

constexpr int ZJ = 12;   // copies per launch
constexpr size_t NONE = ~size_t(0);

// dst[r * ld_d + c] for r < rows_d, c < cols_d  <-  src[r * ld_s + c] where r < rows_s and c < cols_s, else zero.
// Pads ([R,C] -> [Rp,Cp]) and compacts ([R,Cp] -> [R,C]) rows of fp32 (esz 4) or bf16 (esz 2) elements bit for bit.
struct ZCopy {
  const void* src;
  void* dst;
  uint32_t rows_s, cols_s, ld_s, rows_d, cols_d, ld_d, esz;
};
struct ZBatch {
  ZCopy c[ZJ];
};

template <typename E>
__device__ __forceinline__ void zcopy_elems(const ZCopy& j) {
  const E* __restrict__ src = static_cast<const E*>(j.src);
  E* __restrict__ dst = static_cast<E*>(j.dst);
  const uint32_t n = j.rows_d * j.cols_d;               // < 2^30 (zext_route)
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
    const uint32_t r = i / j.cols_d, c = i - r * j.cols_d;
    const bool in = r < j.rows_s && c < j.cols_s;
    const E v = in ? src[(size_t)r * j.ld_s + c] : E(0);
    dst[(size_t)r * j.ld_d + c] = v;
  }
}

__global__ __launch_bounds__(256) void zext_copy(ZBatch b) {
  const ZCopy j = b.c[blockIdx.y];
  if (j.esz == 4) zcopy_elems<uint32_t>(j);
  else zcopy_elems<uint16_t>(j);
}

struct Copies {
  ZBatch b{};
  int n = 0;
  uint32_t maxn = 0;
  int err = FASTGRNN_OK;

  void add(const void* src, void* dst, size_t rs, size_t cs, size_t lds, size_t rd, size_t cd, size_t ldd, size_t esz,
           hipStream_t s) {
    if (n == ZJ) launch(s);
    b.c[n++] = ZCopy{src, dst, (uint32_t)rs, (uint32_t)cs, (uint32_t)lds, (uint32_t)rd, (uint32_t)cd, (uint32_t)ldd,
                     (uint32_t)esz};
    if (rd * cd > maxn) maxn = (uint32_t)(rd * cd);
  }
  // [R,C] -> [Rp,Cp], zero fill
  void pad(const void* src, void* dst, size_t R, size_t C, size_t Rp, size_t Cp, size_t esz, hipStream_t s) {
    add(src, dst, R, C, C, Rp, Cp, Cp, esz, s);
  }
  // [R,Cp] -> [R,C]
  void compact(const void* src, void* dst, size_t R, size_t Cp, size_t C, size_t esz, hipStream_t s) {
    add(src, dst, R, C, Cp, R, C, C, esz, s);
  }
  void launch(hipStream_t s) {
    if (n == 0) return;
    uint32_t bx = (maxn + 255) / 256;
    if (bx > 4096) bx = 4096;
    if (bx == 0) bx = 1;
    hipLaunchKernelGGL(zext_copy, dim3(bx, n), dim3(256), 0, s, b);
    if (hipGetLastError() != hipSuccess) err = FASTGRNN_ERR_LAUNCH;
    n = 0;
    maxn = 0;
  }
};

// Offsets into the caller's workspace (NONE: not needed, the caller's tensor is used as it is).  The padded
// parameters first, then the padded inputs, the padded outputs and the inner path-2 workspace.
struct ZWs {
  size_t w, u, w1, w2, u1, u2, bg, bu;   // padded parameters
  size_t x, h0, seq;                     // padded x, h0; hs (forward) or grad_hs (backward)
  size_t dx, dh0, dw, du, dw1, dw2, du1, du2, dbg, dbu;   // padded gradients (backward)
  size_t inner, total;
};

ZWs zlayout(const fastgrnn_desc& d, const fastgrnn_desc& e, bool backward) {
  const size_t H = d.H, F = d.F, Hp = e.H, Fp = e.F, TB = (size_t)d.T * d.B, B = d.B;
  const size_t rw = d.w_rank, ru = d.u_rank, es = seq_esz(d);
  const bool ph = H != Hp, pf = F != Fp;
  ZWs L;
  size_t o = 0;
  auto take = [&](bool need, size_t bytes) {
    if (!need) return NONE;
    const size_t at = o;
    o += align256(bytes);
    return at;
  };
  L.w = take(!rw && (ph || pf), Hp * Fp * 4);
  L.w1 = take(rw && pf, rw * Fp * 4);
  L.w2 = take(rw && ph, Hp * rw * 4);
  L.u = take(!ru && ph, Hp * Hp * 4);
  L.u1 = take(ru && ph, ru * Hp * 4);
  L.u2 = take(ru && ph, Hp * ru * 4);
  L.bg = take(ph, Hp * 4);
  L.bu = take(ph, Hp * 4);
  L.x = take(pf, TB * Fp * es);
  L.h0 = take(ph, B * Hp * 4);
  const bool preact = (d.flags & FASTGRNN_FLAG_SAVE_PREACT) != 0;
  if (!backward) {
    // hs: into the saved buffer under FASTGRNN_FLAG_SAVE_PREACT, else here ([B,Hp] under FASTGRNN_FLAG_HS_LAST)
    L.seq = take(ph && !preact, ((d.flags & FASTGRNN_FLAG_HS_LAST) ? B : TB) * Hp * es);
    L.dx = L.dh0 = L.dw = L.du = L.dw1 = L.dw2 = L.du1 = L.du2 = L.dbg = L.dbu = NONE;
  } else {
    L.seq = take(ph, ((d.flags & FASTGRNN_FLAG_GRAD_LAST) ? B : TB) * Hp * es);
    L.dx = take(pf, TB * Fp * es);
    L.dh0 = take(ph, B * Hp * 4);
    L.dw = take(!rw && (ph || pf), Hp * Fp * 4);
    L.dw1 = take(rw && pf, rw * Fp * 4);
    L.dw2 = take(rw && ph, Hp * rw * 4);
    L.du = take(!ru && ph, Hp * Hp * 4);
    L.du1 = take(ru && ph, ru * Hp * 4);
    L.du2 = take(ru && ph, Hp * ru * 4);
    L.dbg = take(ph, Hp * 4);
    L.dbu = take(ph, Hp * 4);
  }
  L.inner = o;
  o += backward ? split_backward_ws(e) : split_forward_ws(e);
  L.total = o;
  return L;
}

// The saved buffer of FASTGRNN_FLAG_SAVE_PREACT on this route (z_s, opaque to the caller): the padded pre-activation
// (fp32), the padded hidden-state sequence (sequence dtype; only when H != Hp -- else the caller's hs is it) and the
// rank-space vector of the low-rank scans (fp32 [T*B,32]; only when the padded cell runs on them)
struct ZSaved {
  size_t pre, hs, cs, total;
};
ZSaved zsaved(const fastgrnn_desc& d, const fastgrnn_desc& e) {
  const size_t TB = (size_t)d.T * d.B, Hp = e.H;
  ZSaved S;
  size_t o = 0;
  S.pre = o; o += align256(TB * Hp * 4);
  S.hs = NONE; S.cs = NONE;
  if (d.H != e.H) { S.hs = o; o += align256(TB * Hp * seq_esz(d)); }
  if (family_of(e) == &lowrank_family()) { S.cs = o; o += align256(TB * 32 * 4); }
  S.total = o;
  return S;
}

char* at(void* base, size_t off) { return off == NONE ? nullptr : reinterpret_cast<char*>(base) + off; }

// the padded parameters (a pointer to the caller's own where no padding is needed)
fastgrnn_params pack_params(const fastgrnn_desc& d, const fastgrnn_desc& e, const fastgrnn_params& p, void* ws,
                            const ZWs& L, Copies& q, hipStream_t s) {
  const size_t H = d.H, F = d.F, Hp = e.H, Fp = e.F, rw = d.w_rank, ru = d.u_rank;
  fastgrnn_params r = p;
  auto one = [&](const void* src, size_t off, size_t R, size_t C, size_t Rp, size_t Cp) -> const void* {
    if (off == NONE) return src;
    q.pad(src, at(ws, off), R, C, Rp, Cp, 4, s);
    return at(ws, off);
  };
  if (rw) {
    r.w1 = one(p.w1, L.w1, rw, F, rw, Fp);
    r.w2 = one(p.w2, L.w2, H, rw, Hp, rw);
  } else {
    r.w = one(p.w, L.w, H, F, Hp, Fp);
  }
  if (ru) {
    r.u1 = one(p.u1, L.u1, ru, H, ru, Hp);
    r.u2 = one(p.u2, L.u2, H, ru, Hp, ru);
  } else {
    r.u = one(p.u, L.u, H, H, Hp, Hp);
  }
  r.bias_gate = one(p.bias_gate, L.bg, 1, H, 1, Hp);
  r.bias_update = one(p.bias_update, L.bu, 1, H, 1, Hp);
  return r;   // zeta, nu: the caller's
}

}  // namespace

size_t zext_forward_ws(const fastgrnn_desc& d, const fastgrnn_desc& e) { return zlayout(d, e, false).total; }
size_t zext_backward_ws(const fastgrnn_desc& d, const fastgrnn_desc& e) { return zlayout(d, e, true).total; }
size_t zext_saved_bytes(const fastgrnn_desc& d, const fastgrnn_desc& e) {
  return (d.flags & FASTGRNN_FLAG_SAVE_PREACT) ? zsaved(d, e).total : 0;
}

int zext_forward(const fastgrnn_desc& d, const fastgrnn_desc& e, const fastgrnn_params& p, const void* x,
                 const void* h0, void* hs, void* zs, void* ws, hipStream_t s) {
  const ZWs L = zlayout(d, e, false);
  const size_t H = d.H, F = d.F, Hp = e.H, Fp = e.F, TB = (size_t)d.T * d.B, B = d.B, es = seq_esz(d);
  const bool preact = (d.flags & FASTGRNN_FLAG_SAVE_PREACT) != 0;
  Copies q;
  const fastgrnn_params pp = pack_params(d, e, p, ws, L, q, s);
  const void* xp = x;
  if (L.x != NONE) { q.pad(x, at(ws, L.x), TB, F, TB, Fp, es, s); xp = at(ws, L.x); }
  const void* h0p = h0;
  if (L.h0 != NONE) { q.pad(h0, at(ws, L.h0), B, H, B, Hp, 4, s); h0p = at(ws, L.h0); }
  q.launch(s);
  if (q.err) return q.err;
  void* zp = nullptr;
  void* cp = nullptr;
  void* hsp = hs;
  if (preact) {
    const ZSaved S = zsaved(d, e);
    zp = at(zs, S.pre);
    cp = at(zs, S.cs);
    if (S.hs != NONE) hsp = at(zs, S.hs);
  } else if (L.seq != NONE) {
    hsp = at(ws, L.seq);
  }
  const int st = split_forward(e, pp, xp, h0p, hsp, zp, cp, at(ws, L.inner), s);
  if (st != FASTGRNN_OK) return st;
  if (hsp != hs) {
    q.compact(hsp, hs, (d.flags & FASTGRNN_FLAG_HS_LAST) ? B : TB, Hp, H, es, s);
    q.launch(s);
  }
  return q.err;
}

int zext_backward(const fastgrnn_desc& d, const fastgrnn_desc& e, const fastgrnn_params& p, const void* ghs,
                  const void* x, const void* hs, const void* zs, const void* h0, const fastgrnn_grads& g, void* ws,
                  hipStream_t s) {
  const ZWs L = zlayout(d, e, true);
  const ZSaved S = zsaved(d, e);
  const size_t H = d.H, F = d.F, Hp = e.H, Fp = e.F, TB = (size_t)d.T * d.B, B = d.B, es = seq_esz(d);
  const size_t rw = d.w_rank, ru = d.u_rank;
  Copies q;
  const fastgrnn_params pp = pack_params(d, e, p, ws, L, q, s);
  const void* xp = x;
  if (L.x != NONE) { q.pad(x, at(ws, L.x), TB, F, TB, Fp, es, s); xp = at(ws, L.x); }
  const void* h0p = h0;
  if (L.h0 != NONE) { q.pad(h0, at(ws, L.h0), B, H, B, Hp, 4, s); h0p = at(ws, L.h0); }
  const void* ghsp = ghs;
  if (L.seq != NONE) {
    const size_t R = (d.flags & FASTGRNN_FLAG_GRAD_LAST) ? B : TB;
    q.pad(ghs, at(ws, L.seq), R, H, R, Hp, es, s);
    ghsp = at(ws, L.seq);
  }
  q.launch(s);
  if (q.err) return q.err;
  const void* hsp = S.hs != NONE ? (const void*)at(const_cast<void*>(zs), S.hs) : hs;
  const void* csp = S.cs != NONE ? (const void*)at(const_cast<void*>(zs), S.cs) : nullptr;
  // the padded gradients: into the workspace where their shape differs, else straight into the caller's
  fastgrnn_grads ge = g;
  auto out = [&](void* own, size_t off) -> void* { return off == NONE ? own : at(ws, off); };
  ge.d_x = g.d_x ? out(g.d_x, L.dx) : nullptr;   // (NULL: family::dx_optional, not wanted)
  ge.d_h0 = out(g.d_h0, L.dh0);
  ge.d_w = out(g.d_w, L.dw);
  ge.d_w1 = out(g.d_w1, L.dw1);
  ge.d_w2 = out(g.d_w2, L.dw2);
  ge.d_u = out(g.d_u, L.du);
  ge.d_u1 = out(g.d_u1, L.du1);
  ge.d_u2 = out(g.d_u2, L.du2);
  ge.d_bias_gate = out(g.d_bias_gate, L.dbg);
  ge.d_bias_update = out(g.d_bias_update, L.dbu);
  const int st = split_backward(e, pp, ghsp, xp, hsp, at(const_cast<void*>(zs), S.pre), csp, h0p, ge,
                                at(ws, L.inner), s);
  if (st != FASTGRNN_OK) return st;
  if (g.d_x && L.dx != NONE) q.compact(ge.d_x, g.d_x, TB, Fp, F, es, s);
  if (L.dh0 != NONE) q.compact(ge.d_h0, g.d_h0, B, Hp, H, 4, s);
  if (L.dw != NONE) q.compact(ge.d_w, g.d_w, H, Fp, F, 4, s);      // dW[:H, :F]
  if (L.dw1 != NONE) q.compact(ge.d_w1, g.d_w1, rw, Fp, F, 4, s);  // dW1[:, :F]
  if (L.dw2 != NONE) q.compact(ge.d_w2, g.d_w2, H, rw, rw, 4, s);  // dW2[:H, :]
  if (L.du != NONE) q.compact(ge.d_u, g.d_u, H, Hp, H, 4, s);      // dU[:H, :H]
  if (L.du1 != NONE) q.compact(ge.d_u1, g.d_u1, ru, Hp, H, 4, s);  // dU1[:, :H]
  if (L.du2 != NONE) q.compact(ge.d_u2, g.d_u2, H, ru, ru, 4, s);  // dU2[:H, :]
  if (L.dbg != NONE) q.compact(ge.d_bias_gate, g.d_bias_gate, 1, Hp, H, 4, s);
  if (L.dbu != NONE) q.compact(ge.d_bias_update, g.d_bias_update, 1, Hp, H, 4, s);
  q.launch(s);
  return q.err;
}

}  // namespace fastgrnn
