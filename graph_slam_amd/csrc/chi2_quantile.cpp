// fgo_chi2_quantile: utils::chi2(dof, alpha) of the reference (gtsam/chi2.h:17-26, boost::math::quantile(chi_squared(dof), alpha)),
// the number every gate of this library is compared with.  Host only.  chi-square(dof) at x is the gamma distribution of shape
// a = dof / 2 at x / 2: the regularised lower incomplete gamma function P(a, z) comes from its power series below z = a + 1 and
// from the continued fraction of Q = 1 - P above (modified Lentz), and x is found by a Newton iteration kept inside a bracket.
#include <cmath>
#include <limits>
#include "../../include/fgo.h"

namespace {

// P(a, z) - p, evaluated on the side that carries no cancellation: P - p from the series, (1 - p) - Q from the continued fraction
double gamma_p_minus(double a, double z, double p) {
  const double eps = std::numeric_limits<double>::epsilon();
  const double front = std::exp(a * std::log(z) - z - std::lgamma(a));        // z^a e^-z / Gamma(a)
  if (z < a + 1.0) {
    double term = 1.0 / a, sum = term;
    for (int n = 1; n < 1000; ++n) {
      term *= z / (a + n);
      sum += term;
      if (term < sum * 0.25 * eps) break;
    }
    return front * sum - p;
  }
  const double tiny = 1e-300;
  double b = z + 1.0 - a, c = 1.0 / tiny, d = 1.0 / b, h = d;
  for (int n = 1; n < 1000; ++n) {
    const double an = -n * (n - a);
    b += 2.0;
    d = an * d + b;
    if (std::fabs(d) < tiny) d = tiny;
    c = b + an / c;
    if (std::fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    const double del = d * c;
    h *= del;
    if (std::fabs(del - 1.0) < 0.25 * eps) break;
  }
  return (1.0 - p) - front * h;
}

// the standard normal quantile to about 4.5e-4 (Abramowitz & Stegun 26.2.23): good enough for a start
double normal_quantile_rough(double p) {
  const double q = p < 0.5 ? p : 1.0 - p, t = std::sqrt(-2.0 * std::log(q));
  const double z = t - (2.515517 + t * (0.802853 + t * 0.010328)) / (1.0 + t * (1.432788 + t * (0.189269 + t * 0.001308)));
  return p < 0.5 ? -z : z;
}

}  // namespace

extern "C" double fgo_chi2_quantile(int dof, double p) {
  if (dof < 1) return 0.0;
  if (std::isnan(p)) return p;
  if (p <= 0.0) return 0.0;
  if (p >= 1.0) return std::numeric_limits<double>::infinity();
  const double a = 0.5 * dof;
  // Wilson-Hilferty: (x / dof)^(1/3) is close to normal with mean 1 - 2 / (9 dof) and variance 2 / (9 dof); in the lower tail of a small
  // dof, where that cube turns negative or overshoots, the first term of the series, P = z^a / Gamma(a + 1)
  const double v = 2.0 / (9.0 * dof), w = 1.0 - v + normal_quantile_rough(p) * std::sqrt(v);
  const double small = 2.0 * std::exp((std::log(p) + std::lgamma(a + 1.0)) / a);
  double x = dof * w * w * w;
  if (!(w > 0) || small < 0.1 * dof) x = small;
  double lo = 0.0, hi = std::numeric_limits<double>::infinity();
  for (int it = 0; it < 200; ++it) {
    const double z = 0.5 * x, r = gamma_p_minus(a, z, p);
    if (r == 0) break;
    if (r < 0) lo = x; else hi = x;
    const double pdf = 0.5 * std::exp((a - 1.0) * std::log(z) - z - std::lgamma(a));
    double xn = x - r / pdf;
    if (!(xn > lo && xn < hi)) xn = std::isinf(hi) ? 2.0 * x : 0.5 * (lo + hi);      // Newton left the bracket: bisect (or grow)
    const double step = std::fabs(xn - x);
    x = xn;
    if (step <= 2.0 * std::numeric_limits<double>::epsilon() * x) break;
  }
  return x;
}
