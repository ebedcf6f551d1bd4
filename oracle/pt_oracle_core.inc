/*
 * pt_oracle_core.inc — literal CPU restatement of the reference hot path.
 * TEST INFRASTRUCTURE ONLY (see pt_oracle.h).  Included twice by pt_oracle.c with
 *   ORACLE_LIBM = 0 (deterministic math, NS = det)  and  = 1 (glibc / host semantics, NS = libm).
 *
 * Everything here follows the reference's OWN data layout and control flow
 * (one BVHNode per leaf and per inner node, Shape -> TriangleMesh -> indices ->
 * vertices pointer chase, Hit() recomputing 1/d, full Intersection record on
 * every valid hit, no closest-t pruning), so that the optimised device layout
 * is checked against an independent statement of the algorithm.
 */

#define CAT_(a, b) a##_##b
#define CAT(a, b) CAT_(a, b)
#define FN(name) CAT(name, NS)

#if ORACLE_LIBM
#define OMAX(a, b) o_max_tern((a), (b))     /* torrey.cuh:70-73 template max */
#define OMIN(a, b) o_min_tern((a), (b))     /* torrey.cuh:75-78 template min */
#define OFMAXF(a, b) o_max_tern((a), (b))   /* cutil_math.h:36-39 host fmaxf */
#define OFMINF(a, b) o_min_tern((a), (b))   /* cutil_math.h:31-34 host fminf */
#define OSINCOS(x, s, c) do { *(c) = cosf(x); *(s) = sinf(x); } while (0)
#define OPOWF(x, y) powf((x), (y))
#define OPOW5(x) ((float)pow((double)(x), 5.0))   /* scene.h:335 pow(float,int) -> double pow on the host */
#else
#define OMAX(a, b) o_fmax_ieee((a), (b))
#define OMIN(a, b) o_fmin_ieee((a), (b))
#define OFMAXF(a, b) o_fmax_ieee((a), (b))
#define OFMINF(a, b) o_fmin_ieee((a), (b))
#define OSINCOS(x, s, c) o_det_sincosf((x), (s), (c))
#define OPOWF(x, y) o_det_powf((x), (y))
#define OPOW5(x) o_det_pow5(x)
#endif

/* clamp: cutil_math.h:65-68 */
static inline float FN(clampf)(float f, float a, float b) { return OFMAXF(a, OFMINF(f, b)); }

/* normalize: cutil_math.h:401-405 (v * rsqrtf(dot)); host rsqrtf = 1/sqrtf (cutil_math.h:51-54) */
static inline v3 FN(normalize)(v3 v) {
    float inv_len = 1.0f / sqrtf(v3dot(v, v));
    return v3scale(v, inv_len);
}

/* bbox.cuh:35-61 */
typedef struct { int did_hit; float tnear, tfar; } FN(hit_result);
static inline FN(hit_result) FN(box_hit)(const pt_bvh_node* nd, const o_ray* ray) {
    v3 inv_dir = v3make(1.0f / ray->dir.x, 1.0f / ray->dir.y, 1.0f / ray->dir.z);
    v3 t0 = v3mul(v3sub(v3make(nd->bmin[0], nd->bmin[1], nd->bmin[2]), ray->org), inv_dir);
    v3 t1 = v3mul(v3sub(v3make(nd->bmax[0], nd->bmax[1], nd->bmax[2]), ray->org), inv_dir);
    if (inv_dir.x < 0.0f) { float tmp = t0.x; t0.x = t1.x; t1.x = tmp; }
    if (inv_dir.y < 0.0f) { float tmp = t0.y; t0.y = t1.y; t1.y = tmp; }
    if (inv_dir.z < 0.0f) { float tmp = t0.z; t0.z = t1.z; t1.z = tmp; }
    float tnear = OMAX(OMAX(t0.x, t0.y), t0.z);
    float tfar = OMIN(OMIN(t1.x, t1.y), t1.z);
    FN(hit_result) r;
    r.did_hit = tfar >= OMAX(0.0f, tnear);
    r.tnear = tnear;
    r.tfar = tfar;
    return r;
}

/* shape.cuh:110-133 */
static inline int FN(solve_quadratic)(float a, float b, float c, float* t0, float* t1) {
    if (a == 0) {
        if (b == 0) return 0;
        *t0 = *t1 = -c / b;
        return 1;
    }
    float discriminant = b * b - 4 * a * c;
    if (discriminant < 0) return 0;
    float root_discriminant = sqrtf(discriminant);
    if (b >= 0) {
        *t0 = (-b - root_discriminant) / (2 * a);
        *t1 = 2 * c / (-b - root_discriminant);
    } else {
        *t0 = 2 * c / (-b + root_discriminant);
        *t1 = (-b + root_discriminant) / (2 * a);
    }
    return 1;
}

/* shape.cuh:135-186 (uv dropped: never read downstream, texture.h:69-71) */
static inline int FN(isect_sphere)(const pt_shape* sph, const o_ray* ray, o_isect* out) {
    v3 center = v3make(sph->center[0], sph->center[1], sph->center[2]);
    v3 v = v3sub(ray->org, center);
    float A = v3dot(ray->dir, ray->dir);
    float B = 2 * v3dot(ray->dir, v);
    float C = v3dot(v, v) - sph->radius * sph->radius;
    float t0, t1;
    if (!FN(solve_quadratic)(A, B, C, &t0, &t1)) return 0;
    if (t0 > t1) { float tmp = t0; t0 = t1; t1 = tmp; }
    float t = t0;
    if (t0 >= ray->tnear && t0 < ray->tfar) t = t0;
    if (t1 >= ray->tnear && t1 < ray->tfar && t < ray->tnear) t = t1;
    if (t >= ray->tnear && t < ray->tfar) {
        v3 p = v3add(ray->org, v3scale(ray->dir, t));
        v3 n = FN(normalize)(v3sub(p, center));
        out->position = p;
        out->geometric_normal = n;
        out->shading_normal = n;
        out->distance = t;
        out->material_id = sph->material_id;
        out->area_light_id = sph->area_light_id;
        out->bu = 0; out->bv = 0;
        return 1;
    }
    return 0;
}

/* shape.cuh:188-215 + scene.h:176-224 */
static inline int FN(isect_triangle)(const pt_scene_desc* sc, const pt_shape* tri, const o_ray* ray,
                                     o_isect* out, o_counters* cnt) {
    const pt_mesh* mesh = &sc->meshes[tri->mesh_index];
    const int32_t* idx = &mesh->indices[3 * (size_t)tri->face_index];
    v3 p0 = v3ld(&mesh->positions[3 * (size_t)idx[0]]);
    v3 p1 = v3ld(&mesh->positions[3 * (size_t)idx[1]]);
    v3 p2 = v3ld(&mesh->positions[3 * (size_t)idx[2]]);

    v3 e1 = v3sub(p1, p0);
    v3 e2 = v3sub(p2, p0);
    v3 s1 = v3cross(ray->dir, e2);
    float divisor = v3dot(s1, e1);
    if (divisor == 0) return 0;
    float inv_divisor = 1 / divisor;
    v3 s = v3sub(ray->org, p0);
    float u = v3dot(s, s1) * inv_divisor;
    v3 s2 = v3cross(s, e1);
    float v = v3dot(ray->dir, s2) * inv_divisor;
    float t = v3dot(e2, s2) * inv_divisor;
    if (!(t > ray->tnear && t < ray->tfar && u >= 0 && v >= 0 && u + v <= 1)) return 0;

    (void)cnt;
    float w = 1 - u - v;
    v3 p = v3add(v3add(v3scale(p0, w), v3scale(p1, u)), v3scale(p2, v));
    v3 geometric_normal = FN(normalize)(v3cross(v3sub(p1, p0), v3sub(p2, p0)));
    v3 shading_normal = geometric_normal;
    if (mesh->normals) {
        v3 n0 = v3ld(&mesh->normals[3 * (size_t)idx[0]]);
        v3 n1 = v3ld(&mesh->normals[3 * (size_t)idx[1]]);
        v3 n2 = v3ld(&mesh->normals[3 * (size_t)idx[2]]);
        shading_normal = FN(normalize)(v3add(v3add(v3scale(n0, w), v3scale(n1, u)), v3scale(n2, v)));
    }
    out->position = p;
    out->geometric_normal = geometric_normal;
    out->shading_normal = shading_normal;
    out->distance = t;
    out->material_id = mesh->material_id;
    out->area_light_id = mesh->area_light_id;
    out->bu = u; out->bv = v;
    return 1;
}

/* scene.h:246-301 */
static int FN(intersect)(const pt_scene_desc* sc, const o_ray* ray, o_isect* closest, int* closest_prim,
                         o_counters* cnt) {
    int valid = 0;
    float closestT = FLT_MAX;
    enum { STACK_CAP = 64 };
    int stack[STACK_CAP];
    int sp = 0;
    stack[sp++] = sc->root;
    cnt->segments++;
    while (sp > 0) {
        if (sp >= STACK_CAP) { cnt->stack_overflow++; break; }   /* scene.h:260-263 */
        if ((uint64_t)sp > cnt->max_stack) cnt->max_stack = (uint64_t)sp;
        int cur = stack[--sp];
        const pt_bvh_node* node = &sc->nodes[cur];
        if (node->prim != -1) {
            const pt_shape* sh = &sc->shapes[node->prim];
            o_isect res;
            int hit = 0;
            O_TRACE(cnt, 'L');
            if (sh->type == PT_SHAPE_SPHERE) { cnt->leaf_sphere++; hit = FN(isect_sphere)(sh, ray, &res); }
            else if (sh->type == PT_SHAPE_TRIANGLE) { cnt->leaf_tri++; hit = FN(isect_triangle)(sc, sh, ray, &res, cnt); }
            if (hit) cnt->valid_hits++;
            if (hit && res.distance < closestT) {
                closestT = res.distance;
                *closest = res;
                *closest_prim = node->prim;
                valid = 1;
                cnt->closer_hits++;
                if (sh->type == PT_SHAPE_TRIANGLE) cnt->closer_tri++;
            }
            continue;
        }
        cnt->inner_pops++;
        O_TRACE(cnt, 'I');
        FN(hit_result) lh = FN(box_hit)(&sc->nodes[node->left], ray);
        FN(hit_result) rh = FN(box_hit)(&sc->nodes[node->right], ray);
        if (lh.did_hit && rh.did_hit) {
            if (lh.tnear < rh.tnear) { stack[sp++] = node->right; stack[sp++] = node->left; }
            else { stack[sp++] = node->left; stack[sp++] = node->right; }
        } else {
            if (lh.did_hit) stack[sp++] = node->left;
            if (rh.did_hit) stack[sp++] = node->right;
        }
    }
    return valid;
}

/* scene.h:333-336 */
static inline v3 FN(schlick_fresnel)(v3 F0, float cos_theta) {
    v3 one = v3make(1.0f, 1.0f, 1.0f);
    float p5 = OPOW5(1 - cos_theta);
    if (g_oracle_mutation & PT_ORACLE_MUT_SCHLICK_POW4) { float x = 1 - cos_theta; p5 = (x * x) * (x * x); }   /* test hook */
    return v3add(F0, v3scale(v3sub(one, F0), p5));
}

/* scene.h:338-345 */
static inline v3 FN(sample_cos_hemisphere)(float ux, float uy) {
    float phi = O_TWOPI * ux;
    float tmp = sqrtf(FN(clampf)(1 - uy, 0.0f, 1.0f));
    float sn, cs;
    OSINCOS(phi, &sn, &cs);
    return v3make(cs * tmp, sn * tmp, sqrtf(FN(clampf)(uy, 0.0f, 1.0f)));
}

/* scene.h:348-357 */
static inline v3 FN(sample_cos_n_hemisphere)(float ux, float uy, float exponent) {
    float phi = O_TWOPI * ux;
    float cos_theta = OPOWF(uy, 1.0f / (exponent + 1));
    float sin_theta = sqrtf(FN(clampf)(1 - cos_theta * cos_theta, 0.0f, 1.0f));
    float sn, cs;
    OSINCOS(phi, &sn, &cs);
    return v3make(cs * sin_theta, sn * sin_theta, cos_theta);
}

/* frame.h:17-29, 39-43, 62-64 */
static inline v3 FN(to_world_about)(v3 n, v3 local) {
    v3 fx, fy;
    if (n.z < (float)(-1 + 1e-6)) {
        fx = v3make(0, -1, 0);
        fy = v3make(-1, 0, 0);
    } else {
        float a = 1 / (1 + n.z);
        float b = -n.x * n.y * a;
        fx = v3make(1 - n.x * n.x * a, b, -n.x);
        fy = v3make(b, 1 - n.y * n.y * a, -n.y);
    }
    return v3add(v3add(v3scale(fx, local.x), v3scale(fy, local.y)), v3scale(n, local.z));
}

/* reflect about n: scene.h:381,435,448,458  (-wi + 2*dot(wi,n)*n) */
static inline v3 FN(reflect)(v3 wi, v3 n) {
    float k = 2 * v3dot(wi, n);
    return v3add(v3neg(wi), v3scale(n, k));
}

typedef struct { v3 wo; int is_pure_specular; v3 weight; } FN(sampling_record);

/* scene.h:422-464 */
static inline FN(sampling_record) FN(sample_brdf)(const pt_scene_desc* sc, const o_isect* isect, v3 n, v3 wi,
                                                  o_pcg32* rng, o_counters* cnt) {
    const pt_material* mat = &sc->materials[isect->material_id];
    FN(sampling_record) r;
    r.is_pure_specular = 0;
    r.weight = v3make(0, 0, 0);
    r.wo = v3make(0, 0, 0);
    if (mat->type == PT_MAT_DIFFUSE) {
        float ux = o_pcg_float(rng); float uy = o_pcg_float(rng); cnt->rng_draws += 2;
        r.wo = FN(to_world_about)(n, FN(sample_cos_hemisphere)(ux, uy));
    } else if (mat->type == PT_MAT_MIRROR) {
        v3 wo = FN(reflect)(wi, n);
        v3 F0 = v3ld(mat->reflectance);
        r.wo = wo;
        r.is_pure_specular = 1;
        r.weight = FN(schlick_fresnel)(F0, v3dot(n, wo));
    } else if (mat->type == PT_MAT_PLASTIC) {
        float q = (mat->eta - 1) / (mat->eta + 1);
        float F0s = q * q;
        v3 F = FN(schlick_fresnel)(v3make(F0s, F0s, F0s), v3dot(n, wi));
        float xi = o_pcg_float(rng); cnt->rng_draws += 1;
        if (xi <= F.x) {
            r.wo = FN(reflect)(wi, n);
            r.is_pure_specular = 1;
            r.weight = v3make(1, 1, 1);
        } else {
            float ux = o_pcg_float(rng); float uy = o_pcg_float(rng); cnt->rng_draws += 2;
            r.wo = FN(to_world_about)(n, FN(sample_cos_hemisphere)(ux, uy));
        }
    } else if (mat->type == PT_MAT_PHONG) {
        float ux = o_pcg_float(rng); float uy = o_pcg_float(rng); cnt->rng_draws += 2;
        v3 wo_local = FN(sample_cos_n_hemisphere)(ux, uy, mat->exponent);
        r.wo = FN(to_world_about)(FN(reflect)(wi, n), wo_local);
    }
    return r;
}

/* scene.h:364-412 */
static inline void FN(eval_brdf)(const pt_scene_desc* sc, const o_isect* isect, v3 n, v3 wi, v3 wo,
                                 v3* value, float* pdf) {
    const pt_material* mat = &sc->materials[isect->material_id];
    *value = v3make(0, 0, 0);
    *pdf = 0;
    if (mat->type == PT_MAT_DIFFUSE) {
        float c = OMAX(v3dot(wo, n), 0.0f) / O_PI;
        *value = v3scale(v3ld(mat->reflectance), c);
        if (g_oracle_mutation & PT_ORACLE_MUT_DIFFUSE_NO_INV_PI) *value = v3scale(v3ld(mat->reflectance), OMAX(v3dot(wo, n), 0.0f));   /* test hook */
        *pdf = c;
    } else if (mat->type == PT_MAT_MIRROR) {
        /* zero */
    } else if (mat->type == PT_MAT_PLASTIC) {
        float q = (mat->eta - 1) / (mat->eta + 1);
        float F0s = q * q;
        v3 F = FN(schlick_fresnel)(v3make(F0s, F0s, F0s), v3dot(n, wi));
        float c = OMAX(v3dot(wo, n), 0.0f) / O_PI;
        *value = v3scale(v3mul(v3sub(v3make(1.0f, 1.0f, 1.0f), F), v3ld(mat->reflectance)), c);
        *pdf = (1 - F.x) * c;
    } else if (mat->type == PT_MAT_PHONG) {
        v3 r = FN(reflect)(wi, n);
        float r_dot_wo = v3dot(r, wo);
        float n_dot_wo = v3dot(n, wo);
        if (r_dot_wo > 0 && n_dot_wo > 0) {
            float phong_response = ((mat->exponent + 1) / (2 * O_PI)) * OPOWF(r_dot_wo, mat->exponent);
            *value = v3scale(v3ld(mat->reflectance), phong_response);
            *pdf = phong_response;
        }
    }
}

/* ---- next-event estimation (SURVEY §8f.4) -------------------------------------------------------------------------
 * An EXTENSION: the reference samples no light (emission is picked up only when a BSDF-sampled ray happens to hit an
 * emitter, radiance.cuh:35-43; its point lights are parsed, light.h:5-8, and never used; its occlusion query is dead
 * code, scene.h:306-330).  With PT_RENDER_NEE every non-specular hit also samples ONE light of scene.lights[] uniformly
 * and connects to it with a shadow ray; emission found by BSDF sampling is then counted only on camera rays and after
 * specular bounces, so area lights are not counted twice.  Same expectation as the reference's estimator for scenes lit
 * by area lights (tests/test_nee.py), less noise for small lights; point lights light the scene for the first time.
 * This restatement is the checker for the HIP path's NEE mode (bit for bit); no reference output exists for it. */

/* any hit in (tnear, tfar)?  scene.h:306-330's query, iterative; the result does not depend on the visit order */
static int FN(occluded)(const pt_scene_desc* sc, const o_ray* ray, o_counters* cnt) {
    enum { STACK_CAP = 64 };
    int stack[STACK_CAP];
    int sp = 0;
    stack[sp++] = sc->root;
    cnt->shadow_rays++;
    while (sp > 0) {
        if (sp >= STACK_CAP) { cnt->stack_overflow++; break; }
        int cur = stack[--sp];
        const pt_bvh_node* node = &sc->nodes[cur];
        if (node->prim != -1) {
            const pt_shape* sh = &sc->shapes[node->prim];
            o_isect res;
            int hit = 0;
            if (sh->type == PT_SHAPE_SPHERE) hit = FN(isect_sphere)(sh, ray, &res);
            else if (sh->type == PT_SHAPE_TRIANGLE) hit = FN(isect_triangle)(sc, sh, ray, &res, cnt);
            if (hit) return 1;
            continue;
        }
        FN(hit_result) lh = FN(box_hit)(&sc->nodes[node->left], ray);
        FN(hit_result) rh = FN(box_hit)(&sc->nodes[node->right], ray);
        if (lh.did_hit) stack[sp++] = node->left;
        if (rh.did_hit) stack[sp++] = node->right;
    }
    return 0;
}

/* eval_brdf for the light direction, divided by the probability of the lobe the estimator is in: PLASTIC reaches its
 * diffuse lobe with probability 1 - F.x (scene.h:443-453), which eval_brdf folds into its pdf, not into its value */
static inline v3 FN(nee_brdf)(const pt_scene_desc* sc, const o_isect* isect, v3 n, v3 wi, v3 wl) {
    v3 value; float pdf;
    FN(eval_brdf)(sc, isect, n, wi, wl, &value, &pdf);
    const pt_material* mat = &sc->materials[isect->material_id];
    if (mat->type == PT_MAT_PLASTIC) {
        float q = (mat->eta - 1) / (mat->eta + 1);
        float F0s = q * q;
        v3 F = FN(schlick_fresnel)(v3make(F0s, F0s, F0s), v3dot(n, wi));
        float inv = 1.0f / (1 - F.x);
        if (!(g_oracle_mutation & PT_ORACLE_MUT_NEE_NO_LOBE_WEIGHT))   /* test hook */
            value = v3scale(value, inv);
    }
    return value;
}

/* radiance a BSDF-sampled ray would pick up on primitive `prim` (radiance.cuh:35-43 incl. the parsed-light-id quirk) */
static inline int FN(prim_emission)(const pt_scene_desc* sc, int prim, v3* le) {
    const pt_shape* sh = &sc->shapes[prim];
    int lid = sh->type == PT_SHAPE_SPHERE ? sh->area_light_id : sc->meshes[sh->mesh_index].area_light_id;
    if (lid == -1 || lid >= sc->num_lights) return 0;
    const pt_light* light = &sc->lights[lid];
    if (light->type != PT_LIGHT_DIFFUSE_AREA) return 0;
    *le = v3ld(light->radiance);
    return 1;
}

/* One light sample at hit point p (normal n faces wi).  Draws: 1 (which light) + 2 (where on an area light).
 * Returns 1 with a shadow ray and the radiance to add if it is unoccluded. */
static inline int FN(nee_sample)(const pt_scene_desc* sc, const o_isect* isect, v3 p, v3 n, v3 wi, v3 throughput,
                                 o_pcg32* rng, o_counters* cnt, o_ray* shadow, v3* contrib) {
    const int nl = sc->num_lights;
    if (nl <= 0) return 0;
    float xi = o_pcg_float(rng); cnt->rng_draws += 1;
    int k = (int)(xi * (float)nl);
    if (k > nl - 1) k = nl - 1;
    const pt_light* light = &sc->lights[k];
    v3 x, le;
    float geom;          /* cos_light * area  (1 for a point light) */
    if (light->type == PT_LIGHT_POINT) {
        x = v3ld(light->position);
        le = v3ld(light->radiance);
        geom = 1.0f;
        v3 dv = v3sub(x, p);
        float d2 = v3dot(dv, dv);
        if (!(d2 > 0)) return 0;
        float d = sqrtf(d2);
        float invd = 1.0f / d;
        v3 wl = v3scale(dv, invd);
        v3 f = FN(nee_brdf)(sc, isect, n, wi, wl);
        if (!(OFMAXF(OFMAXF(f.x, f.y), f.z) > 0)) return 0;
        float w = ((float)nl * geom) / d2;
        if (g_oracle_mutation & PT_ORACLE_MUT_NEE_NO_NUM_LIGHTS) w = geom / d2;   /* test hook */
        *contrib = v3mul(throughput, v3scale(v3mul(f, le), w));
        shadow->org = p; shadow->dir = wl; shadow->tnear = 1e-4f; shadow->tfar = d;
        return 1;
    }
    float u1 = o_pcg_float(rng); float u2 = o_pcg_float(rng); cnt->rng_draws += 2;
    const int prim = light->shape_id;
    if (prim < 0 || prim >= sc->num_shapes) return 0;
    if (!FN(prim_emission)(sc, prim, &le)) return 0;
    const pt_shape* sh = &sc->shapes[prim];
    v3 nx;               /* the normal a ray hitting x would see (shading normal) */
    v3 ng;               /* unit geometric normal */
    float area;
    if (sh->type == PT_SHAPE_SPHERE) {
        float z = 1 - 2 * u1;
        float r = sqrtf(FN(clampf)(1 - z * z, 0.0f, 1.0f));
        float phi = O_TWOPI * u2;
        float sn, cs;
        OSINCOS(phi, &sn, &cs);
        nx = v3make(r * cs, r * sn, z);
        ng = nx;
        x = v3add(v3ld(sh->center), v3scale(nx, sh->radius));
        area = (4 * O_PI) * (sh->radius * sh->radius);
    } else {
        const pt_mesh* mesh = &sc->meshes[sh->mesh_index];
        const int32_t* idx = &mesh->indices[3 * (size_t)sh->face_index];
        v3 p0 = v3ld(&mesh->positions[3 * (size_t)idx[0]]);
        v3 p1 = v3ld(&mesh->positions[3 * (size_t)idx[1]]);
        v3 p2 = v3ld(&mesh->positions[3 * (size_t)idx[2]]);
        float su = sqrtf(u1);
        float bu = su * (1 - u2), bv = su * u2, bw = 1 - su;       /* uniform on the triangle */
        x = v3add(v3add(v3scale(p0, bw), v3scale(p1, bu)), v3scale(p2, bv));
        v3 c = v3cross(v3sub(p1, p0), v3sub(p2, p0));
        float len = sqrtf(v3dot(c, c));
        if (!(len > 0)) return 0;
        float invl = 1.0f / len;
        ng = v3scale(c, invl);
        area = 0.5f * len;
        v3 n0 = v3ld(&mesh->normals[3 * (size_t)idx[0]]);
        v3 n1 = v3ld(&mesh->normals[3 * (size_t)idx[1]]);
        v3 n2 = v3ld(&mesh->normals[3 * (size_t)idx[2]]);
        nx = FN(normalize)(v3add(v3add(v3scale(n0, bw), v3scale(n1, bu)), v3scale(n2, bv)));
    }
    v3 dv = v3sub(x, p);
    float d2 = v3dot(dv, dv);
    if (!(d2 > 0)) return 0;
    float d = sqrtf(d2);
    float invd = 1.0f / d;
    v3 wl = v3scale(dv, invd);
    if (!(v3dot(v3neg(wl), nx) > 0) && !(g_oracle_mutation & PT_ORACLE_MUT_NEE_BOTH_SIDES))   /* test hook in the second term */
        return 0;                                       /* radiance.cuh:38: emits towards dot(-ray.dir, n) > 0 only */
    float cosg = fabsf(v3dot(wl, ng));
    if (g_oracle_mutation & PT_ORACLE_MUT_NEE_COS_SHADING) cosg = fabsf(v3dot(wl, nx));   /* test hook */
    geom = cosg * area;
    v3 f = FN(nee_brdf)(sc, isect, n, wi, wl);
    if (!(OFMAXF(OFMAXF(f.x, f.y), f.z) > 0)) return 0;
    float w = ((float)nl * geom) / d2;
    if (g_oracle_mutation & PT_ORACLE_MUT_NEE_NO_NUM_LIGHTS) w = geom / d2;   /* test hook */
    *contrib = v3mul(throughput, v3scale(v3mul(f, le), w));
    shadow->org = p; shadow->dir = wl; shadow->tnear = 1e-4f; shadow->tfar = d * (1.0f - 1e-4f);
    if (g_oracle_mutation & PT_ORACLE_MUT_NEE_TFAR_FULL) shadow->tfar = d;   /* test hook */
    return 1;
}

/* radiance.cuh:21-79 */
static v3 FN(radiance)(const pt_scene_desc* sc, o_ray ray, o_pcg32* rng, int max_depth, int rr_depth, int nee,
                       o_counters* cnt) {
    int count_emission = 1;            /* NEE: emission found by BSDF sampling counts on camera rays and after specular bounces only */
    FN(sampling_record) nee_sampling;
    memset(&nee_sampling, 0, sizeof nee_sampling);
    v3 L = v3make(0, 0, 0);
    v3 throughput = v3make(1.0f, 1.0f, 1.0f);
    v3 background = v3ld(sc->background);
    int depth;
    cnt->paths++;
    for (depth = 0; depth < max_depth; ++depth) {
        o_isect hit;
        int prim = -1;
        if (!FN(intersect)(sc, &ray, &hit, &prim, cnt)) {
            L = v3add(L, v3mul(throughput, background));
            cnt->term_miss++;
            O_TRACE(cnt, 'M');
            break;
        }
        O_TRACE(cnt, 'S');
        v3 p = hit.position;
        v3 n = hit.shading_normal;
        v3 wi = v3neg(ray.dir);
        /* radiance.cuh:35-43: lights[] is indexed with the PARSED light id (SURVEY H5c) */
        if (hit.area_light_id != -1 && hit.area_light_id < sc->num_lights) {
            const pt_light* light = &sc->lights[hit.area_light_id];
            if (light->type == PT_LIGHT_DIFFUSE_AREA) {
                if (v3dot(wi, n) > 0 && count_emission) {
                    L = v3add(L, v3mul(throughput, v3ld(light->radiance)));
                    cnt->emit++;
                }
            }
        }
        if (v3dot(wi, n) < 0) n = v3neg(n);

        if (nee) {
            /* MIRROR has no non-specular lobe; PLASTIC decides below which lobe this bounce is in, so the light sample
             * is drawn now (fixed draw order: light, BSDF, roulette) and used only if the bounce turns out non-specular */
            const pt_material* mat = &sc->materials[hit.material_id];
            o_ray shadow; v3 contrib;
            int have = mat->type != PT_MAT_MIRROR && FN(nee_sample)(sc, &hit, p, n, wi, throughput, rng, cnt, &shadow, &contrib);
            FN(sampling_record) peek;
            /* the BSDF sample is drawn next, exactly as without NEE; a specular PLASTIC bounce discards the light sample */
            peek = FN(sample_brdf)(sc, &hit, n, wi, rng, cnt);
            if (have && !peek.is_pure_specular && !FN(occluded)(sc, &shadow, cnt)) {
                L = v3add(L, contrib);
                cnt->nee_hits++;
            }
            count_emission = peek.is_pure_specular;
            if (g_oracle_mutation & PT_ORACLE_MUT_NEE_COUNT_EMISSION) count_emission = 1;   /* test hook */
            nee_sampling = peek;
        }
        FN(sampling_record) sampling = nee ? nee_sampling : FN(sample_brdf)(sc, &hit, n, wi, rng, cnt);
        if (sampling.is_pure_specular) {
            if (OFMAXF(OFMAXF(sampling.weight.x, sampling.weight.y), sampling.weight.z) > 0) {
                throughput = v3mul(throughput, sampling.weight);
            } else { cnt->term_absorb++; break; }
        } else {
            v3 value; float pdf;
            FN(eval_brdf)(sc, &hit, n, wi, sampling.wo, &value, &pdf);
            if (OFMAXF(OFMAXF(value.x, value.y), value.z) > 0 && pdf > 0) {
                float inv = 1.0f / pdf;                         /* float3 / float: cutil_math.h:349-353 */
                throughput = v3mul(throughput, v3scale(value, inv));
            } else { cnt->term_absorb++; break; }
        }
        ray.org = p; ray.dir = sampling.wo; ray.tnear = 1e-4f; ray.tfar = FLT_MAX;

        if (depth > rr_depth) {
            float q = OMAX(0.5f, 1 - OFMAXF(OFMAXF(throughput.x, throughput.y), throughput.z));
            if (g_oracle_mutation & PT_ORACLE_MUT_RR_FLOOR_QUARTER)   /* test hook: another roulette, the same expectation */
                q = OMAX(0.25f, 1 - OFMAXF(OFMAXF(throughput.x, throughput.y), throughput.z));
            float xi = o_pcg_float(rng); cnt->rng_draws += 1;
            if (xi < q) { cnt->term_rr++; break; }
            float inv = 1.0f / (1 - q);                          /* float3 /= float: cutil_math.h:359-363 */
            if (!(g_oracle_mutation & PT_ORACLE_MUT_RR_NO_WEIGHT))    /* test hook: survivors not re-weighted */
                throughput = v3scale(throughput, inv);
        }
    }
    if (depth >= max_depth) cnt->term_maxdepth++;
    O_TRACE(cnt, 'E');
    return L;
}

/* camera.cuh:45-50 */
static inline o_ray FN(primary_ray)(const pt_render_params* p, float u, float v) {
    v3 tl = v3ld(p->cam_top_left), hz = v3ld(p->cam_horizontal), vt = v3ld(p->cam_vertical), og = v3ld(p->cam_origin);
    v3 d = v3sub(v3sub(v3add(tl, v3scale(hz, u)), v3scale(vt, v)), og);
    o_ray r;
    r.org = og;
    r.dir = FN(normalize)(d);
    r.tnear = 0.0f;
    r.tfar = INFINITY;
    return r;
}

/* main.cu:30-52 for one pixel; rng_mode per pt_oracle.h */
static void FN(render_pixel)(const pt_scene_desc* sc, const pt_render_params* p, int rng_mode, int i, int j,
                             int max_depth, int rr_depth, int accumulate_only, float* out3, o_counters* cnt) {
    int64_t pixel_index = (int64_t)j * p->width + i;
    int64_t stride = p->stream_stride > 0 ? p->stream_stride : p->spp;
    o_pcg32 rng;
    if (rng_mode == PT_ORACLE_RNG_PER_PIXEL) rng = o_pcg_init((uint64_t)pixel_index, p->seed);
    v3 color = v3make(0, 0, 0);
    for (int s = 0; s < p->spp; s++) {
        if (rng_mode == PT_ORACLE_RNG_PER_SAMPLE)
            rng = o_pcg_init((uint64_t)(pixel_index * stride + p->sample_offset + s), p->seed);
        float r0 = o_pcg_float(&rng);
        float u = ((float)i + r0) / (float)p->width;        /* main.cu:41 */
        float r1 = o_pcg_float(&rng);
        float v = ((float)j + r1) / (float)p->height;       /* main.cu:42 */
        cnt->rng_draws += 2;
        o_ray ray = FN(primary_ray)(p, u, v);
        color = v3add(color, FN(radiance)(sc, ray, &rng, max_depth, rr_depth, (p->flags & PT_RENDER_NEE) != 0, cnt));
    }
    if (!accumulate_only) {
        float inv = 1.0f / (float)p->spp;                   /* main.cu:50: float3 / float */
        color = v3scale(color, inv);
    }
    out3[0] = color.x; out3[1] = color.y; out3[2] = color.z;
}

static int FN(intersect_rays)(const pt_scene_desc* sc, const float* rays, int n, float* out_tuv, int32_t* out_prim) {
    o_counters cnt;
    memset(&cnt, 0, sizeof cnt);
    for (int k = 0; k < n; k++) {
        o_ray r;
        r.org = v3ld(&rays[8 * k]); r.dir = v3ld(&rays[8 * k + 3]);
        r.tnear = rays[8 * k + 6]; r.tfar = rays[8 * k + 7];
        o_isect h; int prim = -1;
        if (FN(intersect)(sc, &r, &h, &prim, &cnt)) {
            out_tuv[3 * k] = h.distance; out_tuv[3 * k + 1] = h.bu; out_tuv[3 * k + 2] = h.bv; out_prim[k] = prim;
        } else {
            out_tuv[3 * k] = 0; out_tuv[3 * k + 1] = 0; out_tuv[3 * k + 2] = 0; out_prim[k] = -1;
        }
    }
    return 0;
}

/* The whole Intersection record of the closest hit (intersection.h), not just t: out_hit = {distance, position[3], shading
 * normal[3], geometric normal[3]}, out_ids = {prim, material, area light}; a miss is all 0 / -1. */
static int FN(intersect_rays_full)(const pt_scene_desc* sc, const float* rays, int n, float* out_hit, int32_t* out_ids) {
    o_counters cnt;
    memset(&cnt, 0, sizeof cnt);
    for (int k = 0; k < n; k++) {
        o_ray r;
        r.org = v3ld(&rays[8 * k]); r.dir = v3ld(&rays[8 * k + 3]);
        r.tnear = rays[8 * k + 6]; r.tfar = rays[8 * k + 7];
        o_isect h; int prim = -1;
        float* o = &out_hit[10 * k];
        int32_t* id = &out_ids[3 * k];
        if (FN(intersect)(sc, &r, &h, &prim, &cnt)) {
            o[0] = h.distance;
            o[1] = h.position.x; o[2] = h.position.y; o[3] = h.position.z;
            o[4] = h.shading_normal.x; o[5] = h.shading_normal.y; o[6] = h.shading_normal.z;
            o[7] = h.geometric_normal.x; o[8] = h.geometric_normal.y; o[9] = h.geometric_normal.z;
            id[0] = prim; id[1] = h.material_id; id[2] = h.area_light_id;
        } else {
            for (int c = 0; c < 10; c++) o[c] = 0;
            id[0] = -1; id[1] = -1; id[2] = -1;
        }
    }
    return 0;
}

/* Work of one intersect() call without the primitive tests: which leaves the traversal of scene.h:246-301 reaches (it never
 * prunes, so that does not depend on what the primitives return), as a count and as an order-independent hash of the
 * primitive ids; and the inner pops.  For the tests of "any tree over the same leaf boxes tests the same leaves". */
static int FN(intersect_work_rays)(const pt_scene_desc* sc, const float* rays, int n, uint32_t* out_inner, uint32_t* out_leaf,
                                   uint64_t* out_leaf_set) {
    for (int k = 0; k < n; k++) {
        o_ray r;
        r.org = v3ld(&rays[8 * k]); r.dir = v3ld(&rays[8 * k + 3]);
        r.tnear = rays[8 * k + 6]; r.tfar = rays[8 * k + 7];
        enum { STACK_CAP = 64 };
        int stack[STACK_CAP];
        int sp = 0;
        uint32_t inner = 0, leaves = 0;
        uint64_t set = 0;
        stack[sp++] = sc->root;
        while (sp > 0) {
            if (sp >= STACK_CAP) return PT_ERR_BAD_SCENE;
            const pt_bvh_node* node = &sc->nodes[stack[--sp]];
            if (node->prim != -1) {
                uint64_t h = ((uint64_t)(uint32_t)node->prim + 1u) * 0x9E3779B97F4A7C15ull;
                h ^= h >> 29;
                set += h * 0xBF58476D1CE4E5B9ull;
                leaves++;
                continue;
            }
            inner++;
            FN(hit_result) lh = FN(box_hit)(&sc->nodes[node->left], &r);
            FN(hit_result) rh = FN(box_hit)(&sc->nodes[node->right], &r);
            if (lh.did_hit && rh.did_hit) {
                if (lh.tnear < rh.tnear) { stack[sp++] = node->right; stack[sp++] = node->left; }
                else { stack[sp++] = node->left; stack[sp++] = node->right; }
            } else {
                if (lh.did_hit) stack[sp++] = node->left;
                if (rh.did_hit) stack[sp++] = node->right;
            }
        }
        out_inner[k] = inner; out_leaf[k] = leaves; out_leaf_set[k] = set;
    }
    return 0;
}

#undef OMAX
#undef OMIN
#undef OFMAXF
#undef OFMINF
#undef OSINCOS
#undef OPOWF
#undef OPOW5
#undef FN
#undef CAT
#undef CAT_
