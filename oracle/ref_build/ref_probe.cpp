/*
 * ref_probe.cpp — command-line driver around a HOST build of the reference renderer's own, unmodified sources
 * (scene.h, radiance.cuh, camera.cuh and the parser / BVH builder they pull in).  TEST INFRASTRUCTURE, our own text:
 * every number this program writes comes out of a function of the reference; nothing of it is restated here.
 * Built by oracle/ref_build/Makefile in two flavours (glibc math, and sin/cos/pow of this translation unit bound to
 * oracle/pt_oracle_math.h: det_bind.h).  tests/golden/make_reference_recordings.py runs it; tests read what it recorded.
 *
 *   ref_probe dump    SCENE.xml W H OUT            the Scene after its constructor + CameraRayData for a W x H film
 *   ref_probe render  SCENE.xml W H SPP SEED MODE OUT [THREADS]
 *                                                  MODE per_sample: PCG stream = pixel_index * SPP + s
 *                                                       per_pixel : one stream per pixel, carried across its samples
 *   ref_probe hits    SCENE.xml RAYS OUT           intersect() for explicit rays, n x {org[3], dir[3], tnear, tfar} float32
 *   ref_probe centres SCENE.xml W H OUT            intersect() for the rays through the pixel centres of a W x H film
 *
 * OUT is a flat list of named arrays: "PTRP", then per array  u32 name length, name, u32 type (0 float32, 1 int32),
 * u32 rank, u32 extents[rank], data (little endian).  Exit status 3 with the message on stderr: the reference's own
 * code refused the input (it throws).  SCENE.xml must be an absolute path (the parser changes directory to its folder).
 */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <string>
#include <thread>
#include <vector>

#ifdef PT_REF_DET_MATH
#include "det_bind.h"
#endif

#include "scene.h"
#include "radiance.cuh"
#include "camera.cuh"

namespace {

struct Out {
    FILE* f;
    explicit Out(const char* path) : f(fopen(path, "wb")) {
        if (!f) { fprintf(stderr, "cannot write %s\n", path); exit(2); }
        fwrite("PTRP", 1, 4, f);
    }
    ~Out() { fclose(f); }
    void u32(uint32_t v) { fwrite(&v, 4, 1, f); }
    void put(const std::string& name, uint32_t type, const std::vector<uint32_t>& ext, const void* data) {
        u32((uint32_t)name.size());
        fwrite(name.data(), 1, name.size(), f);
        u32(type);
        u32((uint32_t)ext.size());
        size_t n = 1;
        for (uint32_t e : ext) { u32(e); n *= e; }
        if (n) fwrite(data, 4, n, f);
    }
    void floats(const std::string& name, const std::vector<float>& v, std::vector<uint32_t> ext) { put(name, 0, ext, v.data()); }
    void ints(const std::string& name, const std::vector<int32_t>& v, std::vector<uint32_t> ext) { put(name, 1, ext, v.data()); }
};

void push3(std::vector<float>& v, const float3& a) { v.push_back(a.x); v.push_back(a.y); v.push_back(a.z); }

struct Loaded {
    Scene scene;
    GPUScene gpu;
    explicit Loaded(const char* path) : scene(parse_scene(fs::path(path))) { gpu.copyFrom(scene); }
};

void dump(const Loaded& L, int W, int H, Out& o) {
    const Scene& s = L.scene;
    // shapes: {type, material, light, face, mesh} and {center, radius}; the fields of the other variant are -1 / 0
    std::vector<int32_t> si;
    std::vector<float> sf;
    for (const Shape& sh : s.shapes) {
        if (sh.type == SPHERE) {
            si.insert(si.end(), {(int32_t)sh.type, sh.sphere.material_id, sh.sphere.area_light_id, -1, -1});
            push3(sf, sh.sphere.center);
            sf.push_back(sh.sphere.radius);
        } else {
            si.insert(si.end(), {(int32_t)sh.type, -1, -1, sh.triangle.face_index, sh.triangle.mesh_index});
            sf.insert(sf.end(), {0.f, 0.f, 0.f, 0.f});
        }
    }
    o.ints("shape_ids", si, {(uint32_t)s.shapes.size(), 5});
    o.floats("shape_sphere", sf, {(uint32_t)s.shapes.size(), 4});

    // meshes, from the arrays the renderer reads (the constructor has released the host copies by now)
    std::vector<int32_t> mh;
    for (size_t k = 0; k < s.meshes.size(); k++) {
        const TriangleMesh& m = s.meshes[k];
        mh.insert(mh.end(), {m.material_id, m.area_light_id, m.positions_size, m.indices_size});
        std::vector<float> P, N;
        std::vector<int32_t> I;
        for (int v = 0; v < m.positions_size; v++) { push3(P, m.device_positions[v]); push3(N, m.device_normals[v]); }
        for (int t = 0; t < m.indices_size; t++)
            I.insert(I.end(), {m.device_indices[t].x, m.device_indices[t].y, m.device_indices[t].z});
        std::string pre = "mesh" + std::to_string(k) + "_";
        o.floats(pre + "positions", P, {(uint32_t)m.positions_size, 3});
        o.floats(pre + "normals", N, {(uint32_t)m.positions_size, 3});
        o.ints(pre + "indices", I, {(uint32_t)m.indices_size, 3});
    }
    o.ints("mesh_header", mh, {(uint32_t)s.meshes.size(), 4});

    // materials: type and {reflectance, eta, exponent}; a field the type does not have is 0
    std::vector<int32_t> mt;
    std::vector<float> mf;
    for (const Material& m : s.materials) {
        mt.push_back((int32_t)m.type);
        float3 r = make_float3(0, 0, 0);
        float eta = 0, ex = 0;
        switch (m.type) {
            case DIFFUSE: r = m.diffuse.reflectance; break;
            case MIRROR: r = m.mirror.reflectance; break;
            case PLASTIC: r = m.plastic.reflectance.constant.color; eta = m.plastic.eta; break;
            case PHONG: r = m.phong.reflectance.constant.color; ex = m.phong.exponent; break;
        }
        push3(mf, r);
        mf.push_back(eta);
        mf.push_back(ex);
    }
    o.ints("material_type", mt, {(uint32_t)mt.size()});
    o.floats("material_params", mf, {(uint32_t)mt.size(), 5});

    // lights: {type, shape} and {radiance | intensity, position}
    std::vector<int32_t> lt;
    std::vector<float> lf;
    for (const Light& l : s.lights) {
        if (l.type == DIFFUSEAREALIGHT) {
            lt.insert(lt.end(), {(int32_t)l.type, l.diffusearealight.shape_id});
            push3(lf, l.diffusearealight.radiance);
            lf.insert(lf.end(), {0.f, 0.f, 0.f});
        } else {
            lt.insert(lt.end(), {(int32_t)l.type, -1});
            push3(lf, l.pointlight.intensity);
            push3(lf, l.pointlight.position);
        }
    }
    o.ints("light_ids", lt, {(uint32_t)s.lights.size(), 2});
    o.floats("light_params", lf, {(uint32_t)s.lights.size(), 6});

    // BVH: the pool the renderer traverses
    std::vector<int32_t> ni;
    std::vector<float> nb;
    for (int k = 0; k < L.gpu.num_bvh_nodes; k++) {
        const BVHNode& n = L.gpu.GPU_bvh_nodes[k];
        push3(nb, n.box.p_min);
        push3(nb, n.box.p_max);
        ni.insert(ni.end(), {n.left_node_id, n.right_node_id, n.primitive_id});
    }
    o.floats("node_box", nb, {(uint32_t)L.gpu.num_bvh_nodes, 6});
    o.ints("node_ids", ni, {(uint32_t)L.gpu.num_bvh_nodes, 3});
    o.ints("root", {L.gpu.bvh_root_index, (int32_t)s.CPU_bvh_nodes.size(), computeMaxDepth(s.CPU_bvh_nodes, s.bvh_root_id)}, {3});

    std::vector<float> bg, cam, crd;
    push3(bg, s.background_color);
    o.floats("background", bg, {3});
    push3(cam, s.camera.lookfrom);
    push3(cam, s.camera.lookat);
    push3(cam, s.camera.up);
    cam.push_back(s.camera.vfov);
    o.floats("camera", cam, {10});
    o.ints("film", {s.width, s.height, s.samples_per_pixel}, {3});
    CameraRayData c = compute_camera_ray_data(L.gpu.camera, W, H);
    push3(crd, c.origin);
    push3(crd, c.top_left_corner);
    push3(crd, c.horizontal);
    push3(crd, c.vertical);
    o.floats("camera_ray_data", crd, {4, 3});
    o.ints("camera_ray_data_film", {W, H}, {2});
}

// One pixel: SPP samples, each two jitter draws (u first) and one call of the reference's radiance(); their mean.
float3 pixel(const GPUScene& g, const CameraRayData& c, int W, int H, int i, int j, int spp, uint64_t seed, bool per_pixel) {
    uint64_t index = (uint64_t)j * (uint64_t)W + (uint64_t)i;
    curandState st = init_pcg32(index, seed);
    float3 sum = make_float3(0.0f, 0.0f, 0.0f);
    for (int s = 0; s < spp; s++) {
        if (!per_pixel) st = init_pcg32(index * (uint64_t)spp + (uint64_t)s, seed);
        float du = curand_uniform(&st);
        float u = ((float)i + du) / (float)W;
        float dv = curand_uniform(&st);
        float v = ((float)j + dv) / (float)H;
        sum += radiance(g, generate_primary_ray(c, u, v), st);
    }
    return sum / float(spp);
}

void render(const Loaded& L, int W, int H, int spp, uint64_t seed, bool per_pixel, int threads, Out& o) {
    CameraRayData c = compute_camera_ray_data(L.gpu.camera, W, H);
    std::vector<float> fb((size_t)W * H * 3);
    if (threads < 1) threads = 1;
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; t++)
        pool.emplace_back([&, t] {
            for (int j = t; j < H; j += threads)
                for (int i = 0; i < W; i++) {
                    float3 px = pixel(L.gpu, c, W, H, i, j, spp, seed, per_pixel);
                    float* d = &fb[((size_t)j * W + i) * 3];
                    d[0] = px.x; d[1] = px.y; d[2] = px.z;
                }
        });
    for (auto& th : pool) th.join();
    o.floats("frame", fb, {(uint32_t)H, (uint32_t)W, 3});
}

void hits(const Loaded& L, const std::vector<Ray>& rays, Out& o) {
    size_t n = rays.size();
    std::vector<float> rr, hf;
    std::vector<int32_t> hi;
    for (const Ray& r : rays) {
        push3(rr, r.org);
        push3(rr, r.dir);
        rr.push_back(r.tnear);
        rr.push_back(r.tfar);
        OptionalIntersection h = intersect(L.gpu, r);
        if (h.valid) {
            hf.push_back(h.value.distance);
            push3(hf, h.value.position);
            push3(hf, h.value.shading_normal);
            push3(hf, h.value.geometric_normal);
            hi.insert(hi.end(), {1, h.value.material_id, h.value.area_light_id});
        } else {
            hf.insert(hf.end(), 10, 0.0f);
            hi.insert(hi.end(), {0, -1, -1});
        }
    }
    o.floats("rays", rr, {(uint32_t)n, 8});
    o.floats("hit", hf, {(uint32_t)n, 10});       // distance, position, shading normal, geometric normal
    o.ints("hit_ids", hi, {(uint32_t)n, 3});      // valid, material, area light
}

int run(int argc, char** argv) {
    std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "dump" && argc == 6) {
        Loaded L(argv[2]);
        Out o(argv[5]);
        dump(L, atoi(argv[3]), atoi(argv[4]), o);
    } else if (cmd == "render" && (argc == 9 || argc == 10)) {
        std::string mode = argv[7];
        if (mode != "per_sample" && mode != "per_pixel") { fprintf(stderr, "MODE is per_sample or per_pixel\n"); return 2; }
        Loaded L(argv[2]);
        Out o(argv[8]);
        render(L, atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), strtoull(argv[6], nullptr, 10), mode == "per_pixel",
               argc == 10 ? atoi(argv[9]) : (int)std::thread::hardware_concurrency(), o);
    } else if (cmd == "hits" && argc == 5) {
        Loaded L(argv[2]);
        FILE* f = fopen(argv[3], "rb");
        if (!f) { fprintf(stderr, "cannot read %s\n", argv[3]); return 2; }
        std::vector<Ray> rays;
        float r[8];
        while (fread(r, 4, 8, f) == 8)
            rays.push_back(Ray{make_float3(r[0], r[1], r[2]), make_float3(r[3], r[4], r[5]), r[6], r[7]});
        fclose(f);
        Out o(argv[4]);
        hits(L, rays, o);
    } else if (cmd == "centres" && argc == 6) {
        Loaded L(argv[2]);
        int W = atoi(argv[3]), H = atoi(argv[4]);
        CameraRayData c = compute_camera_ray_data(L.gpu.camera, W, H);
        std::vector<Ray> rays;
        for (int j = 0; j < H; j++)
            for (int i = 0; i < W; i++)
                rays.push_back(generate_primary_ray(c, (float(i) + 0.5f) / float(W), (float(j) + 0.5f) / float(H)));
        Out o(argv[5]);
        hits(L, rays, o);
    } else {
        fprintf(stderr, "usage: ref_probe dump|render|hits|centres ... (see the head of ref_probe.cpp)\n");
        return 2;
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    try {
        return run(argc, argv);
    } catch (const std::exception& e) {
        fprintf(stderr, "REJECTED: %s\n", e.what());
        return 3;
    }
}
