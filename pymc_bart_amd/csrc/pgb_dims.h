// pgb_dims.h -- part of pgbart_hip.hip and of k_loglik_compiled.hip (not a standalone header): the launch geometry
// and record sizes every kernel header relies on.
#define CH 1024 /* rows per chunk = rows per k_rows workgroup */
#define BT 256  /* threads per workgroup */
#define RPT (CH / BT)
#define MAXN PGB_MAX_NODES
#define MAXP PGB_MAX_PARTICLES
#define CC_ROUNDS 256
#define NGEN 8 /* generations of particle leaf labels (ring) */
