// tsim_param_body.h — what the two kernels of the body groups share (link inertia, motors, limits): k_param_grad_body (tsim_param_grad_body.hip),
// which contracts the residual's derivative w.r.t. the body columns with the adjoint solution, and k_tangent_body_src (tsim_tangent_body.hip),
// which contracts it with a direction.  Only those two units include it.
#pragma once
#include "tsim_kernels.h"

// ================================================================================================ body groups
// d/dp of  a . I b  for the spatial inertia I of a link (mass m, world centre of mass cw = XR c + Xp, rotational inertia XR Il XR^T about it):
//     a . I b = m av . bv + a_w^T XR Il XR^T b_w ,   av = a_l + a_w x cw  (the velocity of the centre of mass under the motion a)
// p = 0 mass, 1..3 c (link frame), 4..9 Il (xx yy zz xy xz yz).
template <class R> __device__ __forceinline__ R pgb_dinertia(int p, R m, const M3<R>& XR, V3<R> cw, S6<R> a, S6<R> b) {
  if (p < 4) {
    const V3<R> av = a.l + cross3(a.a, cw), bv = b.l + cross3(b.a, cw);
    if (p == 0) return dot3(av, bv);
    const V3<R> d = cross3(bv, a.a) + cross3(av, b.a);          // d(av . bv) / d cw
    const V3<R> col = p == 1 ? mk3<R>(XR.m[0], XR.m[3], XR.m[6]) : p == 2 ? mk3<R>(XR.m[1], XR.m[4], XR.m[7]) : mk3<R>(XR.m[2], XR.m[5], XR.m[8]);
    return m * dot3(col, d);                                     // d cw / d c = XR
  }
  const V3<R> al = mulMtv(XR, a.a), bl = mulMtv(XR, b.a);
  switch (p) {
    case 4: return al.x * bl.x;
    case 5: return al.y * bl.y;
    case 6: return al.z * bl.z;
    case 7: return al.x * bl.y + al.y * bl.x;
    case 8: return al.x * bl.z + al.z * bl.x;
    default: return al.y * bl.z + al.z * bl.y;
  }
}
