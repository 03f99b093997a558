// facade_fuse.cpp — MapFuser (include/top_down_render/map_fuser.h) on the closed-loop scene of tests/fuse_ref.py: a
// TopDownMapPolar set from the stale label image, scan 0 added from host images, the others rendered by ScanRendererPolar
// from their clouds and added in one addScans; then apply, a second apply, and what the class refuses.  Inputs: raw
// little-endian files in argv[1] (tests/test_fuse.py).  Writes the renders, the votes and the fused labels back, prints
// "ok <changed cells>".
#include <cstdio>
#include <fstream>
#include <memory>
#include <string>

#include "top_down_render/map_fuser.h"
#include "top_down_render/scan_renderer_polar.h"
#include "top_down_render/top_down_map_polar.h"

template <class T>
static std::vector<T> slurp(const std::string& path) {
  std::ifstream in(path, std::ios::binary | std::ios::ate);
  if (!in) throw std::runtime_error("cannot open " + path);
  std::vector<T> v((size_t)in.tellg() / sizeof(T));
  in.seekg(0);
  in.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
  return v;
}
template <class T>
static void dump(const std::string& path, const T* data, size_t n) {
  std::ofstream out(path, std::ios::binary);
  out.write(reinterpret_cast<const char*>(data), (std::streamsize)(n * sizeof(T)));
  if (!out) throw std::runtime_error("cannot write " + path);
}
#define EXPECT(cond)                                                      \
  do {                                                                    \
    if (!(cond)) throw std::runtime_error(std::string("failed: ") + #cond); \
  } while (0)

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s <dir>\n", argv[0]); return 2; }
  const std::string dir = argv[1];
  try {
    int ncls, h, w, nb, nr, n_poses;
    float res;
    uint32_t min_votes, num, den;
    {
      std::ifstream meta(dir + "/meta.txt");
      meta >> ncls >> h >> w >> nb >> nr >> res >> min_votes >> num >> den >> n_poses;
      if (!meta) throw std::runtime_error("bad meta.txt");
    }
    const float ang_res = (float)(2 * M_PI / nb);
    auto labels = slurp<uint8_t>(dir + "/labels.bin");
    auto lut = slurp<int32_t>(dir + "/lut.bin");
    auto poses = slurp<float>(dir + "/poses.bin");   // [n_poses][3]: x, y, theta
    EXPECT(labels.size() == (size_t)h * w && lut.size() == 256 && poses.size() == (size_t)3 * n_poses && n_poses >= 2);

    TopDownMap::Params params;
    params.num_classes = ncls;
    params.resolution = 1.f;
    for (int i = 0; i < 256; i++) params.flatten_lut.push_back(lut[i]);
    TopDownMapPolar map(params);
    map.samplePtsPolar(Eigen::Vector2i(nb, nr), ang_res);
    std::vector<uint8_t> class_label(ncls);
    for (int c = 0; c < ncls; c++) class_label[c] = (uint8_t)c;

    bool threw = false;   // a map that was not set from a label image has no fuser
    try { MapFuser none(map, class_label, min_votes, {num, den}); } catch (const std::runtime_error&) { threw = true; }
    EXPECT(threw);
    map.updateMap(labels.data(), h, w, Eigen::Vector2i(0, 0));
    threw = false;
    try { MapFuser bad(map, class_label, 0, {num, den}); } catch (const std::runtime_error&) { threw = true; }
    EXPECT(threw);
    MapFuser fuser(map, class_label, min_votes, {num, den});

    // scan 0: host images
    auto scan0 = slurp<float>(dir + "/scan_0.bin");
    EXPECT(scan0.size() == (size_t)ncls * nb * nr);
    std::vector<Eigen::ArrayXXf> imgs(ncls, Eigen::ArrayXXf(nb, nr));
    for (int c = 0; c < ncls; c++) std::memcpy(imgs[c].data(), scan0.data() + (size_t)c * nb * nr, (size_t)nb * nr * sizeof(float));
    MapFuser::Pose p0;
    p0.x = poses[0]; p0.y = poses[1]; p0.theta = poses[2];
    EXPECT(fuser.addImages(imgs, true, p0, res) && fuser.lastVotesAdded() > 0);
    dump(dir + "/out_scan_0.bin", scan0.data(), scan0.size());
    // a refused scan: no exception, false, the reason in tdr_last_error()
    std::vector<Eigen::ArrayXXf> wrong(ncls, Eigen::ArrayXXf(nb + 1, nr));
    EXPECT(!fuser.addImages(wrong, true, p0, res) && std::string(tdr_last_error()).find("table") != std::string::npos);
    MapFuser::Pose nan_pose = p0;
    nan_pose.x = std::nanf("");
    EXPECT(!fuser.addImages(imgs, true, nan_pose, res));

    // the other scans: rendered on the device, added in one launch
    Eigen::VectorXi flatten = Eigen::VectorXi::Constant(256, -1);
    for (int i = 0; i < 256; i++) flatten[i] = lut[i];
    std::vector<std::unique_ptr<ScanRendererPolar>> renderers;
    std::vector<const ScanRenderer*> rptr;
    std::vector<MapFuser::Pose> rposes;
    std::vector<float> rres;
    ScanRendererPolar empty(flatten);
    EXPECT(!fuser.addScan(empty, p0, res));   // no render yet
    for (int k = 1; k < n_poses; k++) {
      auto pts = slurp<float>(dir + "/pts_" + std::to_string(k) + ".bin");   // [n][4]: x, y, z, label
      pcl::PointCloud<PointType>::Ptr cloud(new pcl::PointCloud<PointType>());
      for (size_t i = 0; i + 3 < pts.size(); i += 4) {
        PointType p{};
        p.x = pts[i]; p.y = pts[i + 1]; p.z = pts[i + 2]; p.intensity = pts[i + 3];
        cloud->push_back(p);
      }
      renderers.emplace_back(new ScanRendererPolar(flatten));
      std::vector<Eigen::ArrayXXf> r(ncls, Eigen::ArrayXXf(nb, nr));
      renderers.back()->renderSemanticTopDown(cloud, res, ang_res, r);
      std::vector<float> flat((size_t)ncls * nb * nr);
      for (int c = 0; c < ncls; c++) std::memcpy(flat.data() + (size_t)c * nb * nr, r[c].data(), (size_t)nb * nr * sizeof(float));
      dump(dir + "/out_scan_" + std::to_string(k) + ".bin", flat.data(), flat.size());
      rptr.push_back(renderers.back().get());
      MapFuser::Pose p;
      p.x = poses[3 * k]; p.y = poses[3 * k + 1]; p.theta = poses[3 * k + 2];
      rposes.push_back(p);
      rres.push_back(res);
    }
    EXPECT(fuser.addScans(rptr, rposes, rres) && fuser.lastVotesAdded() > 0);
    std::vector<const ScanRenderer*> twice = {rptr[0], rptr[0]};
    EXPECT(!fuser.addScans(twice, {rposes[0], rposes[0]}, {res, res}));   // a renderer twice

    int vc = 0, vr = 0, vcols = 0, ih = 0, iw = 0;
    auto votes = fuser.votes(&vc, &vr, &vcols);
    EXPECT(vc == ncls && vr == h && vcols == w);
    const int64_t changed = fuser.apply();
    EXPECT(changed > 0 && fuser.apply() == 0);
    auto fused = fuser.labels(&ih, &iw);
    EXPECT(ih == h && iw == w);
    dump(dir + "/out_votes.bin", votes.data(), votes.size());
    dump(dir + "/out_labels.bin", fused.data(), fused.size());
    // decay to nothing: every verdict falls back to the base image
    fuser.decay(31);
    EXPECT(fuser.apply() == changed);
    EXPECT(fuser.labels() == labels && fuser.rebase());   // (the map has the fuser's grid: the votes are kept)
    std::printf("ok %lld\n", (long long)changed);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
