/*
 * image_fuzz_main.c -- loader safety of the chain image, as a stand-alone host program (its own main; built with
 * -fsanitize=address,undefined by tests/test_chain_image.py and run as a child process, never loaded into Python).
 *
 *   image_fuzz_main CASE IMAGE N_EDITS SEED
 *
 * CASE:  int64 sizeof(pgb_settings) | pgb_settings | X[n][p] | y[n] | int32 rules[p] (padded to 8 bytes) | prior[p] |
 *        int64 has_offset | offset[K][n] (if has_offset)              -- the arrays a sampler of the case is given
 * IMAGE: a good image of that case (pgb_checkpoint_save).
 *
 * Every edit is applied to a fresh copy of the good record: a single byte XORed, or a whole field replaced by a value
 * that is special for its type, in a section drawn uniformly (so that the small sections -- the header, the node
 * tables -- get as many edits as the large ones).  The edited record goes to pgb_checkpoint_load.  Whatever is
 * ACCEPTED is stepped for two asteps (one tuning, one drawing), exported and saved again: an accepted record is a
 * chain, and a chain must run.  The program exits 0 when nothing crashed (the sanitizers abort otherwise) and no
 * accepted record failed to step; it prints how many edits were accepted.
 */
#include "../oracle/pgbart_oracle.c"

#include <inttypes.h>
#include <stddef.h>

static uint64_t rng_state;
static uint64_t rnd(void) { /* splitmix64 */
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static void* read_file(const char* path, int64_t* bytes) {
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
  fseek(f, 0, SEEK_END);
  *bytes = (int64_t)ftell(f);
  fseek(f, 0, SEEK_SET);
  void* p = malloc((size_t)*bytes + 8);
  if (fread(p, 1, (size_t)*bytes, f) != (size_t)*bytes) { fprintf(stderr, "short read of %s\n", path); exit(2); }
  fclose(f);
  return p;
}

typedef struct { const char* name; int64_t off, elems; int width; int is_float; } section;

static double special_double(void) {
  static const double v[] = {0.0, -0.0, 1.0, -1.0, 1e300, -1e300, 4.9e-324, 1e-300, 255.0, 1e9};
  const uint64_t k = rnd() % 14;
  if (k < 10) return v[k];
  if (k == 10) return __builtin_nan("");
  if (k == 11) return __builtin_inf();
  if (k == 12) return -__builtin_inf();
  uint64_t bits = rnd();
  double d;
  memcpy(&d, &bits, 8);
  return d;
}

static int64_t special_int(int width, int64_t n) {
  const uint64_t k = rnd() % 12;
  const int64_t big = width == 4 ? INT32_MAX : INT64_MAX;
  switch (k) {
    case 0: return -1;
    case 1: return 0;
    case 2: return 1;
    case 3: return n;
    case 4: return n + 1;
    case 5: return big;
    case 6: return -big - 1;
    case 7: return 254;
    case 8: return 255;
    case 9: return (int64_t)(rnd() % 300);
    case 10: return (int64_t)1 << 33;
    default: return (int64_t)rnd();
  }
}

int main(int argc, char** argv) {
  if (argc != 5) { fprintf(stderr, "usage: %s CASE IMAGE N_EDITS SEED\n", argv[0]); return 2; }
  int64_t cbytes = 0, ibytes = 0;
  char* cs = (char*)read_file(argv[1], &cbytes);
  uint8_t* good = (uint8_t*)read_file(argv[2], &ibytes);
  const int n_edits = atoi(argv[3]);
  rng_state = (uint64_t)strtoull(argv[4], NULL, 10);

  int64_t ssz;
  memcpy(&ssz, cs, 8);
  if (ssz != (int64_t)sizeof(pgb_settings)) { fprintf(stderr, "settings size\n"); return 2; }
  pgb_settings st;
  memcpy(&st, cs + 8, sizeof st);
  const int64_t n = st.n;
  const int p = st.p, K = st.n_outputs;
  const char* q = cs + 8 + sizeof st;
  const double* X = (const double*)q; q += 8 * n * p;
  const double* y = (const double*)q; q += 8 * n;
  const int32_t* rules = (const int32_t*)q; q += pgb_image_pad8(4 * (int64_t)p);
  const double* prior = (const double*)q; q += 8 * (int64_t)p;
  int64_t has_off;
  memcpy(&has_off, q, 8); q += 8;
  const double* off = has_off ? (const double*)q : NULL;
  if (has_off) q += 8 * (int64_t)K * n;
  if (q - cs != cbytes) { fprintf(stderr, "case file size\n"); return 2; }

  pgb_handle* h = NULL;
  if (pgb_create(&st, NULL, &h) != PGB_OK || pgb_set_data(h, X, p, rules, prior) != PGB_OK ||
      pgb_set_response(h, y) != PGB_OK || (off && pgb_set_offset(h, off) != PGB_OK)) {
    fprintf(stderr, "setup: %s\n", pgb_last_error());
    return 2;
  }
  if (pgb_checkpoint_load(h, good, ibytes) != PGB_OK) { fprintf(stderr, "the good image: %s\n", pgb_last_error()); return 2; }

  pgb_image_header hd;
  memcpy(&hd, good, sizeof hd);
  pgb_image_view v;
  pgb_image_bind(good, &hd, &v);
  const int64_t N = hd.total_nodes, m = st.m;
#define SEC(nm, ptr, cnt, w, fl) {nm, (int64_t)((const uint8_t*)(ptr) - good), (int64_t)(cnt), w, fl}
  const section secs[] = {
      SEC("header", good, sizeof(pgb_image_header), 1, 0),
      SEC("header.cursor", good + offsetof(pgb_image_header, iter), 2, 8, 0),
      SEC("header.lower", good + offsetof(pgb_image_header, lower), 4, 4, 0),
      SEC("header.leaf_sd", good + offsetof(pgb_image_header, leaf_sd), PGB_MAX_OUTPUTS + 2, 8, 1),
      SEC("header.ctr", good + offsetof(pgb_image_header, ctr), sizeof(pgb_counters) / 8, 8, 0),
      SEC("sum_trees", v.sum_trees, K * n, 8, 1), SEC("rs_mean", v.rs_mean, K * n, 8, 1), SEC("rs_m2", v.rs_m2, K * n, 8, 1),
      SEC("alpha", v.alpha, p, 8, 0), SEC("cdf", v.cdf, p, 8, 0), SEC("node_off", v.node_off, m + 1, 4, 0),
      SEC("var", v.var, N, 4, 0), SEC("left", v.left, N, 4, 0), SEC("right", v.right, N, 4, 0),
      SEC("depth", v.depth, N, 4, 0), SEC("label", v.label, N, 4, 0), SEC("svar", v.svar, N, 4, 0),
      SEC("count", v.count, N, 8, 0), SEC("split", v.split, N, 8, 1), SEC("xbar", v.xbar, N, 8, 1),
      SEC("value", v.value, N * K, 8, 1), SEC("slope", v.slope, N * K, 8, 1), SEC("lid", v.lid, m * n, 1, 0),
  };
  const int n_secs = (int)(sizeof secs / sizeof secs[0]);

  uint8_t* rec = (uint8_t*)malloc((size_t)ibytes); /* exactly the record: a read past it is a sanitizer report */
  double* st_out = (double*)malloc(sizeof(double) * (size_t)n * K);
  int32_t* vi = (int32_t*)malloc(sizeof(int32_t) * (size_t)p);
  int64_t cap = 1 << 20;
  uint8_t* pack = (uint8_t*)malloc((size_t)cap);
  uint8_t* again = (uint8_t*)malloc((size_t)ibytes * 2 + (1 << 20));
  int accepted = 0, step_errors = 0;
  for (int e = 0; e < n_edits; ++e) {
    memcpy(rec, good, (size_t)ibytes);
    const section* s = &secs[rnd() % (uint64_t)n_secs];
    const int64_t el = (int64_t)(rnd() % (uint64_t)s->elems);
    uint8_t* at = rec + s->off + el * s->width;
    const int whole = s->width > 1 && (rnd() & 1);
    if (!whole) {
      at[rnd() % (uint64_t)s->width] ^= (uint8_t)(1 + rnd() % 255);
    } else if (s->is_float) {
      const double d = special_double();
      memcpy(at, &d, 8);
    } else if (s->width == 8) {
      const int64_t x = special_int(8, n);
      memcpy(at, &x, 8);
    } else {
      const int32_t x = (int32_t)special_int(4, n);
      memcpy(at, &x, 4);
    }
    int64_t lbytes = ibytes;
    if (rnd() % 50 == 0) lbytes = (int64_t)(rnd() % (uint64_t)ibytes); /* a truncated record now and then */
    uint8_t* given = rec;
    if (lbytes != ibytes) { /* (its own allocation: a read past the given size is a sanitizer report) */
      given = (uint8_t*)malloc((size_t)lbytes + 1);
      memcpy(given, rec, (size_t)lbytes);
    }
    const int lrc = pgb_checkpoint_load(h, given, lbytes);
    if (given != rec) free(given);
    if (lrc != PGB_OK) continue;
    accepted += 1;
    pgb_counters ctr;
    int rc = pgb_step_host(h, 1, st_out, vi, &ctr);
    if (rc == PGB_OK) rc = pgb_step_host(h, 0, st_out, vi, &ctr);
    int64_t nb = 0;
    if (rc == PGB_OK) {
      rc = pgb_export_trees_packed(h, 1, pack, cap, &nb);
      if (rc == PGB_E_NOMEM) {
        cap = nb * 2;
        pack = (uint8_t*)realloc(pack, (size_t)cap);
        rc = pgb_export_trees_packed(h, 1, pack, cap, &nb);
      }
    }
    if (rc == PGB_OK) rc = pgb_export_trees_packed(h, 0, pack, cap, &nb);
    int64_t sb = 0;
    if (rc == PGB_OK) rc = pgb_checkpoint_size(h, &sb);
    if (rc == PGB_OK && sb <= ibytes * 2 + (1 << 20)) rc = pgb_checkpoint_save(h, again, sb);
    if (rc != PGB_OK) {
      step_errors += 1;
      fprintf(stderr, "edit %d (%s[%" PRId64 "], %s): accepted, then: %s\n", e, s->name, el, whole ? "field" : "byte", pgb_last_error());
    }
  }
  printf("edits %d accepted %d failed_after_accept %d\n", n_edits, accepted, step_errors);
  pgb_destroy(h);
  free(rec); free(st_out); free(vi); free(pack); free(again); free(cs); free(good);
  return step_errors ? 1 : 0;
}
