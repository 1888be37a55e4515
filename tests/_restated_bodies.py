"""The built-in per-row families restated as bodies of the compiled family, operation for operation: run as family
"compiled" they are the SAME sampler as the built-in family (the built-in families clamp at 0 from above, the compiled
family at 2047: hence the closing ``ll > 0.0 ? 0.0 : ll``).  Param order = the case's ``lik_params``."""

POISSON = """double yy = y > 0.0 ? y : 0.0;  double em = exp(mu);
double sat = yy > 0.0 ? yy * log(yy) - yy : 0.0;
double ll = (yy * mu - em) - sat;  return ll > 0.0 ? 0.0 : ll;"""
PROBIT = "return log_ndtr(y > 0.5 ? mu : -mu);"
PROBIT_AUX = "return log_ndtr(aux > 0.5 ? mu : -mu);"  # (aux = the 0/1 response: the body ignores y)
LOGIT = "double ll = -softplus(-(y > 0.5 ? mu : -mu));  return ll > 0.0 ? 0.0 : ll;"
NEGBIN = """double yy = y > 0.0 ? y : 0.0;  double em = exp(mu);  double ay = alpha + yy;
double l1 = log(yy > 0.0 ? yy : alpha);
double sat = yy > 0.0 ? yy * l1 - ay * log(ay) : -(alpha * l1);
double ll = (yy * mu - ay * log(alpha + em)) - sat;  return ll > 0.0 ? 0.0 : ll;"""
GAMMA1 = """double yy = y > 1.0e-300 ? y : 1.0e-300;
double ll = -alpha * (((yy * exp(-mu) + mu) - 1.0) - log(yy));  return ll > 0.0 ? 0.0 : ll;"""
STUDENT = """double u = (y - mu) / sigma;
double ll = (-0.5 * (nu + 1.0)) * log(1.0 + (u * u) / nu);  return ll > 0.0 ? 0.0 : ll;"""
CHECK_LOSS = "double u = (y - mu) / b;  return -(u * (u < 0.0 ? q - 1.0 : q));"
# pgb_loglik_meanscale_t and pgb_loglik_cat_t (tests/test_compiled_kvector.py)
MEANSCALE = """double sd = mu[1] < 0.0 ? -mu[1] : mu[1];
if (!(sd >= 1e-8)) sd = 1e-8;
if (sd > 1.0e300) sd = 1.0e300;
double z = (y - mu[0]) / sd;
return -log(sd) - 0.5 * (z * z);"""
SOFTMAX = """double mx = mu[0];
for (int k = 1; k < K; ++k) if (mu[k] > mx) mx = mu[k];
double sum = 0.0;
for (int k = 0; k < K; ++k) sum += exp(mu[k] - mx);
int c = (int)y;
if (c < 0) c = 0;
if (c > K - 1) c = K - 1;
double muc = mu[0];
for (int k = 1; k < K; ++k) if (k == c) muc = mu[k];
double ll = (muc - mx) - log(sum);
if (!(sum >= 1.0)) ll = -2047.0;
return ll > 0.0 ? 0.0 : ll;"""
SOFTMAX_AUX = SOFTMAX.replace("int c = (int)y;", "int c = (int)aux;")  # (the class read from the aux column)

#: built-in family -> (body, param names in the order of lik_params)
RESTATED = {
    "bernoulli_probit": (PROBIT, ()),
    "bernoulli_logit": (LOGIT, ()),
    "poisson_log": (POISSON, ()),
    "negbin_log": (NEGBIN, ("alpha",)),
    "asymmetric_laplace": (CHECK_LOSS, ("b", "q")),
    "student_t": (STUDENT, ("sigma", "nu")),
    "gamma_log": (GAMMA1, ("alpha",)),
    "normal_meanscale": (MEANSCALE, ()),
    "categorical": (SOFTMAX, ()),
}
