// Generator of the stress-recovery fixtures tests/golden/stress/*.npz (run by
// make_stress_golden.sh on a machine that has the reference; NOT part of the product or of the
// test run).  It includes the reference's headers by path, builds two meshes with the reference's
// own classes, runs the reference's TRANSFER (PATCH), STIF_MATR (elatMatr) and STRESS_RECOVERY on
// a synthetic smooth displacement, and records as raw little-endian arrays in the output
// directory: the element tree as ddpca_multigrid_create takes it (coordinates before PATCH),
// nodeRota, the material, the displacement handed to STRESS_RECOVERY (node ids, solver frame) and
// the reference's resuStre_0.txt.
//   beam         the reference's tapered, twisted BEAM mesh (MESH_NODD), divisions 4 x 2 x 2,
//                one global refinement: 128 non-affine leaf elements, 225 nodes
//   hanging_rot  a smoothly distorted 2 x 2 x 2 box, refined once uniformly, then the corner
//                octant (the 8 children of element 0) refined by REFINE: edge and face hanging
//                nodes on the hanging level; nodeRota on the nodes of the face x = 0 (node-dependent
//                rotations), mateElas = 110e9, matePois = 0.25
// usage: make_stress_golden <case> <outdir>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <fstream>

#include "examples/BEAM.h"

namespace {

template <typename T>
void dump(const std::string& dir, const std::string& name, const std::vector<T>& v) {
    std::ofstream f(dir + "/" + name, std::ios::binary);
    f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}

Eigen::Matrix3d rotation(long node) {
    return Eigen::AngleAxisd(0.3 + 0.01 * (double)node, Eigen::Vector3d(1.0, 2.0, 3.0).normalized()).toRotationMatrix();
}

// a smooth, non-polynomial displacement of amplitude a
Eigen::Vector3d field(const COOR& c, double a, double k) {
    const double x = k * c[0], y = k * c[1], z = k * c[2];
    return Eigen::Vector3d(a * std::sin(1.1 * x + 0.3) * std::sin(0.7 * y + 0.2) * std::cos(0.9 * z),
                           a * std::cos(0.8 * x) * std::sin(1.3 * y + 0.5) * std::sin(0.6 * z + 0.1),
                           a * std::sin(0.5 * x + 0.7) * std::cos(1.2 * y) * std::sin(1.4 * z + 0.4));
}

void record_tree(const MULTIGRID& g, const std::string& dir) {
    std::vector<double> xyz(3 * g.nodeCoor.size());
    for (const auto& nc : g.nodeCoor)
        for (int a = 0; a < 3; ++a) xyz[3 * nc.first + a] = nc.second[a];
    std::vector<int64_t> corner, parent, level, patt, cptr{0}, child;
    for (const auto& e : g.elemVect) {
        for (int k = 0; k < 8; ++k) corner.push_back(e.cornNode[k]);
        parent.push_back(e.parent);
        level.push_back(e.level);
        patt.push_back(e.refiPatt);
        for (long c : e.children) child.push_back(c);
        cptr.push_back((int64_t)child.size());
    }
    dump(dir, "coords.f64", xyz);
    dump(dir, "corner.i64", corner);
    dump(dir, "parent.i64", parent);
    dump(dir, "level.i64", level);
    dump(dir, "refiPatt.i64", patt);
    dump(dir, "child_ptr.i64", cptr);
    dump(dir, "child.i64", child);
}

// TRANSFER (PATCH) + STIF_MATR + STRESS_RECOVERY on u = R^T field(x) at rotated nodes, field(x) elsewhere
void recover(MULTIGRID& g, const std::string& dir, double amp, double k) {
    record_tree(g, dir);
    std::vector<int64_t> rn;
    std::vector<double> rm;
    for (const auto& kv : g.nodeRota) {
        rn.push_back(kv.first);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) rm.push_back(kv.second(i, j));
    }
    dump(dir, "rot_node.i64", rn);
    dump(dir, "rot.f64", rm);
    dump(dir, "material.f64", std::vector<double>{g.mateElas, g.matePois});
    g.TRANSFER();
    g.STIF_MATR();
    Eigen::VectorXd u(3 * g.nodeCoor.size());
    for (const auto& nc : g.nodeCoor) {
        Eigen::Vector3d v = field(nc.second, amp, k);  // coordinates after PATCH
        const auto it = g.nodeRota.find(nc.first);
        if (it != g.nodeRota.end()) v = it->second.transpose() * v;
        u.segment<3>(3 * nc.first) = v;
    }
    dump(dir, "u.f64", std::vector<double>(u.data(), u.data() + u.size()));
    outpDire = dir + "/";
    g.STRESS_RECOVERY(u, 0);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const std::string mode = argv[1], dir = argv[2];
    mkdir(dir.c_str(), 0777);
    if (mode == "beam") {
        BEAM beam(0);
        beam.diviNumb = {4, 2, 2};
        beam.globLeve = 1;
        beam.MESH_NODD(0);
        recover(beam.multGrid[0], dir, 1.0e-4 * 0.01, 6.0);
    } else if (mode == "hanging_rot") {
        MULTIGRID g;
        const int n = 2;
        long id[n + 1][n + 1][n + 1];
        for (int k = 0; k <= n; ++k)
            for (int j = 0; j <= n; ++j)
                for (int i = 0; i <= n; ++i) {
                    const double x = 0.5 * i, y = 0.5 * j, z = 0.5 * k;
                    id[i][j][k] = g.TRY_ADD_NODE(COOR(x + 0.04 * std::sin(2.0 * y + 0.3) * std::cos(1.5 * z),
                                                      y + 0.05 * std::sin(1.7 * z + 0.1) * std::cos(2.2 * x + 0.4),
                                                      z + 0.03 * std::sin(2.4 * x + 0.2) * std::sin(1.9 * y + 0.6)));
                }
        for (int k = 0; k < n; ++k)
            for (int j = 0; j < n; ++j)
                for (int i = 0; i < n; ++i) {
                    TREE_ELEM t;
                    t.parent = -1;
                    t.cornNode = {id[i][j][k],         id[i + 1][j][k],         id[i + 1][j + 1][k],     id[i][j + 1][k],
                                  id[i][j][k + 1],     id[i + 1][j][k + 1],     id[i + 1][j + 1][k + 1], id[i][j + 1][k + 1]};
                    t.level = 0;
                    t.refiPatt = 7;
                    t.children.resize(0);
                    g.ADD_ELEMENT(t);
                }
        std::set<long> split;
        for (long e = 0; e < (long)g.elemVect.size(); ++e) split.insert(e), g.elemVect[e].refiPatt = 0;
        g.REFINE(split, {}, {});
        split.clear();
        for (long c : g.elemVect[0].children) split.insert(c), g.elemVect[c].refiPatt = 0;
        g.REFINE(split, {}, {});
        g.mateElas = 110.0e9;
        g.matePois = 0.25;
        for (const auto& nc : g.nodeCoor)
            if (std::abs(nc.second[0] - 0.04 * std::sin(2.0 * nc.second[1] + 0.3) * std::cos(1.5 * nc.second[2])) < 0.06)
                g.nodeRota.emplace(nc.first, rotation(nc.first));
        recover(g, dir, 1.0e-4 * 0.25, 3.0);
    } else {
        return 2;
    }
    return 0;
}
