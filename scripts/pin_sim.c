/*
 * pin_sim.c — measurement tooling (not a test, not the product): how much of phase C runs at
 * the entry's own carry-in?  For every DEP entry that hits at its exact carry-in (from the CPU
 * oracle) it replays shade_dep_cont's control flow (rc_device.hpp), as phasec_sim.c does, and
 * counts, bit for bit (never ==): the levels that start at the carry-in, the hit levels whose
 * hit point is the carry-in again, the lit-light evaluations and shadow tests whose ray starts
 * there; and, with the entries in k_dep_chunks' order (1 024-entry chunks, hit entries
 * compacted in order, 64 per wave), the waves with one carry-in in every lane and the runs of
 * equal carry-ins per wave.  These are the numbers behind phase C's carry-point table
 * (rc_device.hpp pin_build).
 *
 *   gcc -O2 -ffp-contract=off -Iinclude -Ioracle -Iraytracing-programs_amd/csrc \
 *       scripts/pin_sim.c raytracing-programs_amd/csrc/rc_scene.c -lm -o /tmp/pin_sim
 *   /tmp/pin_sim tests/golden/scenes/quadric.scene 4096 7
 */
#include "../oracle/rc_oracle.c"

#include <stdio.h>

typedef struct {
  long long levels, levels_at_c, hits, hits_at_c, lights, lights_at_c, shadow, shadow_at_c;
} cnt_t;

static int same_bits3(const float *a, const float *b) { return memcmp(a, b, 12) == 0; }

static int refl(const octx *c, int obj) { return c->shapes[obj].reflectivity > 0.0f; }

/* shadow tests until the first hit (the GPU's shadowed() stops there) */
static int shadow_tests(octx *c, const float *P, const float *D, int skip) {
  int n = 0;
  for (int k = 0; k < c->n; k++) {
    if (k == skip) continue;
    ++n;
    float t = 0.0f;
    int h = 0;
    const shape_t *s = &c->shapes[k];
    if (s->type == SPHERE) h = o_sphere(P, D, s, &t);
    else if (s->type == PLANE) h = o_plane(P, D, s, &t);
    else if (s->type == QUADRIC) {
      h = o_quadric(P, D, s, &t);
      if (h && skip != -1 && (P[2] + t * D[2]) < P[2]) h = 0;
    }
    if (h && t > 0.0f && t < INFINITY) return n;
  }
  return n;
}

/* returns whether some level hit */
static int replay(octx *c, const float *A, const float *N0, int obj0, int maxrec, const float *cin,
                  cnt_t *k) {
  float O[3] = {cin[0], cin[1], cin[2]}, C[3] = {cin[0], cin[1], cin[2]};
  float D[3] = {A[0], A[1], A[2]}, N[3] = {N0[0], N0[1], N0[2]};
  int obj = obj0, S = -1, any = 0;
  cnt_t e;
  memset(&e, 0, sizeof e);
  for (int lvl = 2; lvl < maxrec; ++lvl) {
    if (!refl(c, obj)) break;
    if (lvl > 2) {
      float t[3];
      o_reflect(t, D, N);
      o_normalize(c, D, t);
    }
    e.levels++;
    e.levels_at_c += same_bits3(O, cin);
    float P[3], Nn[3];
    const int i = o_nearest(c, O, D, P, Nn, S, 0);
    if (i >= 0) {
      any = 1;
      memcpy(C, P, sizeof C);
      memcpy(N, Nn, sizeof N);
      obj = i;
      const int at_c = same_bits3(P, cin);
      e.hits++;
      e.hits_at_c += at_c;
      const shape_t *o = &c->shapes[i];
      const float opacity = (float)((1.0 - (double)o->reflectivity) - (double)o->refractivity);
      if (opacity > 0.0f) {
        for (int l = 0; l < c->m; l++) {
          const light_t *L = &c->lights[l];
          float ld[3] = {L->position[0] - C[0], L->position[1] - C[1], L->position[2] - C[2]};
          o_normalize(c, ld, ld);
          const float th = o_dot(N, ld);
          if (th <= 0.0f) continue;   /* inert: no shadow ray */
          const int n = shadow_tests(c, C, ld, i);
          e.lights++;
          e.shadow += n;
          if (at_c) e.lights_at_c++, e.shadow_at_c += n;
        }
      }
    }
    memcpy(O, C, sizeof O);
    S = i;
  }
  if (any) {   /* clean entries never reach the second pass */
    k->levels += e.levels, k->levels_at_c += e.levels_at_c, k->hits += e.hits;
    k->hits_at_c += e.hits_at_c, k->lights += e.lights, k->lights_at_c += e.lights_at_c;
    k->shadow += e.shadow, k->shadow_at_c += e.shadow_at_c;
  }
  return any;
}

static double pct(long long a, long long b) { return b ? 100.0 * (double)a / (double)b : 0.0; }

int main(int argc, char **argv) {
  if (argc < 4) return 2;
  json_data_t js;
  if (rco_load_scene(argv[1], &js)) return 1;
  const int W = atoi(argv[2]), H = W, maxrec = atoi(argv[3]);
  const size_t P = (size_t)W * H;
  uint8_t *img = malloc(P * 3), *cls = malloc(P);
  float *cin = malloc(P * 3 * sizeof(float));
  rco_stats st;
  if (rco_render_cls(&js, W, H, maxrec, RCO_MODE_PARITY, img, &st, cin, cls)) return 1;
  octx c;
  memset(&c, 0, sizeof c);
  rco_stats st2;
  memset(&st2, 0, sizeof st2);
  c.st = &st2;
  c.n = js.num_shapes;
  c.m = js.num_lights;
  shape_t *sh = calloc(c.n, sizeof(shape_t));
  light_t *li = calloc(c.m > 0 ? c.m : 1, sizeof(light_t));
  const shape_t *s = js.shapes_list;
  for (int k = 0; k < c.n; k++, s = s->next) sh[k] = *s;
  const light_t *l = js.lights_list;
  for (int k = 0; k < c.m; k++, l = l->next) li[k] = *l;
  c.shapes = sh;
  c.lights = li;
  o_build_phantom(&c);
  const float ph = js.camera_height / (float)H, pw = js.camera_width / (float)W;
  long long ndep = 0;
  for (size_t p = 0; p < P; ++p) ndep += cls[p] >= 2;
  char *hitm = calloc((size_t)ndep + 1, 1);
  const float **cp = malloc(sizeof(float *) * ((size_t)ndep + 1));
  cnt_t k;
  memset(&k, 0, sizeof k);
  long long j = 0, nhit = 0;
  for (size_t p = 0; p < P; ++p) {
    if (cls[p] < 2) continue;
    const int x = (int)(p % W), y = (int)(p / W);
    float d[3];
    d[0] = (float)((0.0 - (double)js.camera_width / 2.0) + (double)pw * ((double)x + 0.5));
    d[1] = (float)((0.0 + (double)js.camera_height / 2.0) - (double)ph * ((double)y + 0.5));
    d[2] = -1.0f;
    o_normalize(&c, d, d);
    float P0[3], N0[3], t[3], D1[3], A[3];
    const float O0[3] = {0, 0, 0};
    const int i0 = o_nearest(&c, O0, d, P0, N0, -1, 0);
    o_reflect(t, d, N0);
    o_normalize(&c, D1, t);
    o_reflect(t, D1, N0);
    o_normalize(&c, A, t);
    hitm[j] = (char)replay(&c, A, N0, i0, maxrec, &cin[3 * p], &k);
    cp[j] = &cin[3 * p];
    nhit += hitm[j];
    ++j;
  }
  /* k_dep_chunks' order: per 1024-entry chunk, the hit entries in order, 64 per wave */
  long long waves = 0, uniform = 0, runs = 0;
  const float **lst = malloc(sizeof(float *) * 1024);
  for (long long ch = 0; ch < ndep; ch += 1024) {
    int n = 0;
    for (long long q = ch; q < ch + 1024 && q < ndep; ++q)
      if (hitm[q]) lst[n++] = cp[q];
    for (int w0 = 0; w0 < n; w0 += 64) {
      const int nw = n - w0 < 64 ? n - w0 : 64;
      int r = 1;
      for (int q = 1; q < nw; ++q) r += !same_bits3(lst[w0 + q], lst[w0 + q - 1]);
      ++waves;
      uniform += r == 1;
      runs += r;
    }
  }
  printf("%s %dx%d maxrec %d: %d shapes, %d lights, DEP entries %lld, hit entries %lld\n", argv[1],
         W, H, maxrec, c.n, c.m, ndep, nhit);
  printf("levels that start at the carry-in        %lld of %lld (%.1f %%)\n", k.levels_at_c, k.levels,
         pct(k.levels_at_c, k.levels));
  printf("hit levels whose hit point is the carry-in %lld of %lld (%.1f %%)\n", k.hits_at_c, k.hits,
         pct(k.hits_at_c, k.hits));
  printf("lit-light evaluations at the carry-in    %lld of %lld (%.1f %%)\n", k.lights_at_c, k.lights,
         pct(k.lights_at_c, k.lights));
  printf("shadow tests from the carry-in           %lld of %lld (%.1f %%)\n", k.shadow_at_c, k.shadow,
         pct(k.shadow_at_c, k.shadow));
  printf("waves with one carry-in in every lane    %lld of %lld (%.1f %%); carry runs per wave %.2f\n",
         uniform, waves, pct(uniform, waves), waves ? (double)runs / (double)waves : 0.0);
  return 0;
}
