"""Sampler bodies shared by ``test_ppc_compiled.py`` (host builds) and ``test_ppc_compiled_gpu.py`` (the device).

``RESTATED``: the formulas of ``pgb_ppc_value`` (``include/pgbart_ppc.h``) written as sampler bodies, in its order of
operations -- case name of ``test_ppc_gpu.CASES`` -> (the body, its param names).  The first call of every kind has
salt 0, so each reproduces the built-in family bit for bit.  (``exp`` is the table exponential without
``pgb_ppc_exp``'s guard beyond +-800, which the predictors of the tests never reach.)"""
import numpy as np

from pymc_bart_amd.compiled import compile_sampler

RESTATED = {
    "normal": ("return mu + s * normal();", ("s",)),
    "normal_meanscale": ("""double sd = mu[1] < 0.0 ? -mu[1] : mu[1];
if (!(sd >= 1e-8)) sd = 1e-8;
if (sd > 1.0e300) sd = 1.0e300;
return mu[0] + sd * normal();""", ()),
    "bernoulli_probit": ("return uniform() < exp(log_ndtr(mu)) ? 1.0 : 0.0;", ()),
    "bernoulli_logit": ("return uniform() < exp(-softplus(-mu)) ? 1.0 : 0.0;", ()),
    "categorical": ("""double mx = mu[0];
for (int k = 1; k < K; ++k)
  if (mu[k] > mx) mx = mu[k];
double sum = 0.0;
for (int k = 0; k < K; ++k) sum = sum + exp(mu[k] - mx);
const double target = uniform() * sum;
double cum = 0.0;
int cls = K - 1;
for (int k = 0; k < K - 1; ++k) {
  cum = cum + exp(mu[k] - mx);
  if (target < cum) {
    cls = k;
    break;
  }
}
return (double)cls;""", ()),
    "asymmetric_laplace": ("""const double u = uniform_open();
if (u < q) return mu + (b / (1.0 - q)) * log(u / q);
return mu - (b / q) * log((1.0 - u) / (1.0 - q));""", ("b", "q")),
    "gamma_log": ("return (exp(mu) * gamma(a)) / a;", ("a",)),
    "student_t": ("""const double h = 0.5 * nu;
const double w = gamma(h) / h;
const double z = normal();
if (w >= 2.2250738585072014e-308 && w <= 1.7976931348623157e308) return mu + (s * z) / sqrt(w);
return z < 0.0 ? -1.0e308 * 10.0 : 1.0e308 * 10.0;""", ("s", "nu")),
    "poisson_log": ("return poisson(exp(mu));", ()),
    "negbin_log": ("return poisson((exp(mu) * gamma(a)) / a);", ("a",)),
}
OUTPUTS = {"normal_meanscale": 2, "categorical": 3}

ZIP = ("return uniform() < pi ? 0.0 : poisson(exp(mu));", ("pi",))          # zero-inflated Poisson
ZIP_AUX = ("return uniform() < pi + aux ? 0.0 : poisson(exp(mu));", ("pi",))  # ... its inflation shifted per row
HETERO = ("return mu[0] + exp(0.5 * mu[1]) * (s * normal());", ("s",))      # K = 2: a mean and a log variance
LOOP3 = ("double t = 0.0;\nfor (int j = 0; j < 3; ++j) t = t + normal() * uniform();\nreturn mu + t;", ())
DIFFERENCE = ("return normal() - normal();", ())
LOOP1025 = ("double t = 0.0;\nfor (int j = 0; j < 1025; ++j) t = t + normal();\nreturn mu + t;", ())
OVERFLOW = ("return (aux > 0.5 ? -1.0 : 1.0) * (1.0e308 * (10.0 + mu * mu));", ())
CENSORED_DENSITY = ("double z = (y - mu) / s; return aux > 0.5 ? log_ndtr(-z) : -0.5*z*z - log(s) - 0.9189385332046727;")
LATENT = "return mu + s * normal();"

_BUILDS = {}


def build(body_and_names, K: int = 1):
    """The build of ``(body, names)``, made once per session."""
    body, names = body_and_names
    key = (body, tuple(names), K)
    if key not in _BUILDS:
        _BUILDS[key] = compile_sampler(body, names, K)
    return _BUILDS[key]


def restated(case: str):
    return build(RESTATED[case], OUTPUTS.get(case, 1))


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float64).view(np.uint64)
