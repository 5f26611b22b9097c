// qg_contact_eval.inc -- contact_eval() of qg_step_dev.h's contact section, textually included twice: at global scope as the template
// every kernel uses (QG_TEMPLATE_T = `template <class T>`, T = float or f2), and inside namespace pk3 as a plain float function
// (QG_TEMPLATE_T empty, T a typedef of float there), where the V3 operators are the packed (x, y) + z overloads -- the one-link-per-lane
// kernel calls that one.  Same text, same arithmetic, same rounding.
QG_TEMPLATE_T DEV void contact_eval(T wsum, V3T<T> s, const FrT<T> &E, V3T<T> p, V3T<T> n, SVT<T> v, float kc, float cmax, float inv_ramp, float mu, float h,
                      SVT<T> &f_ext, ContactDampT<T> &cd) {
    const T zero = T(0.f);
    auto active = wsum > zero;
    T W = kc * wsum;
    T cc = cmax * min_(wsum * inv_ramp, T(1.f));
    T inv = rcp(sel(active, wsum, T(1.f)));
    V3T<T> P = p + rot(E, inv * s);         // centre of pressure, FRAME axes about the FRAME origin
    V3T<T> vP = QG_CROSS_ADD(v.a, P, v.l);        // v.l + v.a x P (the includer says how: plain, or the packed accumulate form)
    T vn = dot(n, vP);
    V3T<T> vt = vP - vn * n;
    T Fn0 = W - cc * vn;
    auto lifted = Fn0 < zero;                // no adhesion: the secant damping coefficient replaces c (vn > 0 here)
    T Fn = sel(lifted, zero, Fn0);
    T cn = sel(lifted, W * rcp(vn), cc);
    T speed = sqrt_(dot(vt, vt));
    auto sliding = cc * speed > mu * Fn;     // Coulomb limit (speed > 0 here)
    T ct = sel(sliding, mu * Fn * rcp(speed), cc);
    Fn = sel(active, Fn, zero);
    cn = sel(active, cn, zero);
    ct = sel(active, ct, zero);
    V3T<T> F = Fn * n - ct * vt;
    f_ext.a = cross(P, F);
    f_ext.l = F;
    cd.mc = h * ct;
    cd.w = h * (cn - ct);
    cd.P = P;
}
