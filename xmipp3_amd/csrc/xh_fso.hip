// xh_fso.hip -- the device side of xmipp_resolution_fso, the Fourier Shell Occupancy (reconstruction/resolution_fso.{h,cpp}, ProgFSO; the
// reference runs on CPU threads only): the global FSC of two half maps, the directional FSCs through Gaussian-weighted cones, the 3DFSC.
//
//   load         the half maps times the mask, two fp64 r2c transforms with the reference's 1 / N, then the reference's compacted,
//                shell-sorted layout (defineFrequencies :111-205, arrangeFSC_and_fscGlobal :209-349): the coefficients with f <= 0.5
//                without the two conjugate-redundant sets of :181-193, ordered by shell round(f X) and, inside a shell, by their raster
//                (k, i, j) order. A position is a pure function of the box: the raster is cut into chunks of FSO_CHUNK elements, one
//                wave counts the kept elements of a chunk per shell, an exclusive scan over the chunks of each shell gives the chunk's
//                first slot, and the same wave walks its chunk again in raster order and hands out the slots. Which lanes of a step share
//                a shell comes from ballots; no atomic takes part. Per kept coefficient: float fx, fy, fz (:295-297), freqidx, arr2indx,
//                float real(conj(z1) z2), |z1|^2, |z2|^2 (:310-312). The per-shell sums of :314-316 are taken in fp64 from the spectra,
//                through arr2indx, by the fixed-order tree of xh_reduce.h, one workgroup per shell;
//   directional  fscDir_fast :428-457 for every direction at once: a workgroup stages one segment (at most `seg` consecutive sorted
//                coefficients of one shell) in LDS, lane d of wave d / 64 walks it for direction d: the cosine and the test in float in the
//                reference's order, the weight by expf, the three products widened to fp64 (exact) and added to fp64 registers. A second
//                kernel adds the segments of each (shell, direction) in increasing order. No floating-point atomics: two runs give the
//                same bytes. Lanes are dealt to directions in spatially compact tiles of 64, so that whole waves skip the coefficients
//                their cones all miss (docs/experiments.md);
//   threedfsc    :492-507 and :1501-1539 with one thread per coefficient, the directions in ascending order, the float accumulation as
//                written (the product w fsc formed in double, then the add, then the rounding to float); NaN -> 1; the scatter through
//                arr2indx, the two line fixes, getCompleteFourier (:1264-1294) and CenterFFT (:1302) for the full map.
//
// Left out, and why nothing changes:
//  - CenterFFT of the half maps (:1030-1031) multiplies both spectra by the same unit-modulus phase: real(conj(z1) z2), |z1|^2 and |z2|^2
//    do not change, and nothing else of the spectra is used;
//  - the DC coefficient is sorted position 0. The reference gives it fx = fy = fz = 0 inf = NaN (the float of DBL_MIN is 0, 1 / f is inf),
//    so its comparison with cosAngle is false for every direction. It is left out of every segment. Its outputs never reach a file: shells
//    0 .. 4 of the FSO are set to 1 (:1469-1470), the directional resolution needs i > 2, and its 3DFSC voxel (0 / 0 = NaN -> 1) is
//    overwritten by the line fix;
//  - aniFilter, the realGaussianFilter of :1548 and the transforms of directionalFilterHalves: that function multiplies both spectra by 1
//    (:1130-1131), so filteredHalfMap{1,2}.mrc are the masked half maps; the program writes those.
// Kept as written: axis frequency 0 is DBL_MIN (:124, :130, :136); the shell index and the f > 0.5 test of :284-288 use 1 / (1 / f), the
// value that went through freqMap; (float) ux * iun is the float of ux times the double iun, rounded to float on assignment.
// Deviation: the sums are fp64 where the reference's float den1 den2 (:468) can overflow on un-normalised spectra.
// Refused: a side below 8 or above 1024; an odd X beside an even Y or Z (a coefficient with f = 0.5 exactly has shell round(X / 2) = X / 2 + 1,
// one past the reference's arrays); the 3DFSC of a box that is not cubic (createFullFourier passes (X, Y, Z) to a (Z, Y, X) resize).
#include "xh_volume.h"
#include "xh_reduce.h"
#include <algorithm>
#include <array>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <map>

namespace {

struct FsoSeg { int start, len; };
struct FsoCoef { float x, y, z, r, a, b; };   // a staged coefficient of the cone kernel

constexpr int FSO_CHUNK = 4096;        // raster elements per chunk of the layout (one wave, 64 steps)
constexpr int FSO_SEG_DEFAULT = 512;   // tools/bench_fso.py: cones + segment reduction 1.03 ms at 256^3 against 1.06 (256, 1024) and 1.36 (2048)
constexpr int FSO_SEG_MAX = 2048;      // 48 KiB of LDS
constexpr int FSO_MAX_DIR = 1024;      // one lane per direction, one workgroup of at most 16 waves
enum { FSO_T_TRANSFORMS = 0, FSO_T_LAYOUT, FSO_T_CONES, FSO_T_SEGREDUCE, FSO_T_3DFSC, FSO_NT };

// defineFrequencies :124-140: the digital frequency of an axis index, DBL_MIN at 0
__device__ __forceinline__ double fso_axis(int idx, int size) { return idx == 0 ? DBL_MIN : d_digfreq(idx, size); }

// raster element e of the half spectrum: is it kept (:173-193, :284), and its shell (:288), axis frequencies and 1 / f (:179)
__device__ __forceinline__ bool fso_elem(size_t e, XhDims d, int &shell, double &uz, double &uy, double &ux, double &iun)
{
    int k, i, j;
    xh_kij(e, d, k, i, j);
    uz = fso_axis(k, d.Z); uy = fso_axis(i, d.Y); ux = fso_axis(j, d.X);
    const double uz2 = uz * uz;
    const double uz2y2 = uz2 + uy * uy;
    const double f = sqrt(uz2y2 + ux * ux);
    if (!(f <= 0.5)) return false;
    if ((j == 0 && uy < 0) || (i == 0 && j == 0 && uz < 0)) return false;
    iun = 1 / f;
    const double f2 = 1 / iun;
    if (f2 > 0.5) return false;
    shell = (int)round(f2 * d.X);
    return shell <= d.X / 2;      // always, for the boxes xh_fso_create accepts: no index can leave the shell arrays
}

// prepareData :1013-1024
__global__ void __launch_bounds__(256) k_fso_mask(const double *__restrict__ v, const double *__restrict__ m, double *__restrict__ out, size_t N)
{
    XH_GRID_LOOP(n, N) out[n] = v[n] * m[n];
}

// one wave per chunk. FILL false: counts [L][nchunks] <- the kept elements of the chunk per shell. FILL true: counts holds the first slot
// of (shell, chunk); the wave hands out the slots in raster order and writes the layout
template <bool FILL>
__global__ void __launch_bounds__(64)
k_fso_layout(const xh_cd *__restrict__ F1, const xh_cd *__restrict__ F2, size_t NF, XhDims d, int L, int nchunks, int *__restrict__ counts,
             float *__restrict__ fx, float *__restrict__ fy, float *__restrict__ fz, int *__restrict__ freqidx, int *__restrict__ arr2indx,
             float *__restrict__ rz, float *__restrict__ a1, float *__restrict__ a2)
{
    extern __shared__ int fso_run[];
    const int lane = threadIdx.x, c = blockIdx.x;
    for (int s = lane; s < L; s += 64) fso_run[s] = FILL ? counts[(size_t)s * nchunks + c] : 0;
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1;
    for (int step = 0; step < FSO_CHUNK / 64; ++step) {
        const size_t e = (size_t)c * FSO_CHUNK + (size_t)step * 64 + lane;
        int shell = -1;
        double uz = 0, uy = 0, ux = 0, iun = 0;
        const bool kept = e < NF && fso_elem(e, d, shell, uz, uy, ux, iun);
        unsigned long long todo = __ballot(kept);
        int pos = -1;
        while (todo) {                                   // one round per distinct shell of the step, the lowest lane's first
            const int leader = __ffsll((long long)todo) - 1;
            const int s0 = __shfl(shell, leader);
            const bool mine = kept && shell == s0;
            const unsigned long long m = __ballot(mine);
            if (mine) pos = fso_run[s0] + __popcll(m & below);
            __syncthreads();
            if (lane == leader) fso_run[s0] += __popcll(m);
            __syncthreads();
            todo &= ~m;
        }
        if (FILL && kept) {
            const xh_cd z1 = F1[e], z2 = F2[e];
            fx[pos] = (float)((double)(float)ux * iun);
            fy[pos] = (float)((double)(float)uy * iun);
            fz[pos] = (float)((double)(float)uz * iun);
            freqidx[pos] = shell;
            arr2indx[pos] = (int)e;
            const double absz1 = hypot(z1.x, z1.y), absz2 = hypot(z2.x, z2.y);
            rz[pos] = (float)(z1.x * z2.x + z1.y * z2.y);
            a1[pos] = (float)((double)(float)absz1 * absz1);
            a2[pos] = (float)((double)(float)absz2 * absz2);
        }
    }
    if (!FILL)
        for (int s = lane; s < L; s += 64) counts[(size_t)s * nchunks + c] = fso_run[s];
}

// per shell (one workgroup): counts [shell][*] -> its exclusive scan, total [shell] <- the shell's size. Thread t owns a run of consecutive
// chunks
__global__ void __launch_bounds__(256) k_fso_scan(int *__restrict__ counts, int nchunks, int *__restrict__ total)
{
    __shared__ int part[256];
    int *row = counts + (size_t)blockIdx.x * nchunks;
    const int per = (nchunks + 255) / 256, t = threadIdx.x;
    const int lo = min(nchunks, t * per), hi = min(nchunks, lo + per);
    int s = 0;
    for (int c = lo; c < hi; ++c) s += row[c];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        int acc = 0;
        for (int q = 0; q < 256; ++q) { const int v = part[q]; part[q] = acc; acc += v; }
        total[blockIdx.x] = acc;
    }
    __syncthreads();
    int acc = part[t];
    for (int c = lo; c < hi; ++c) { const int v = row[c]; row[c] = acc; acc += v; }
}

// counts [shell][chunk] += cumpos [shell] (:217-223)
__global__ void __launch_bounds__(256) k_fso_add_cumpos(int *__restrict__ counts, int nchunks, const int *__restrict__ cumpos)
{
    for (int c = threadIdx.x; c < nchunks; c += 256) counts[(size_t)blockIdx.x * nchunks + c] += cumpos[blockIdx.x];
}

// :314-316 in fp64, one workgroup per shell over its sorted range: thread t adds positions t, t + 256, .. in increasing order, then the tree
__global__ void __launch_bounds__(256)
k_fso_shell_sums(const xh_cd *__restrict__ F1, const xh_cd *__restrict__ F2, const int *__restrict__ arr2indx, const int *__restrict__ cumpos,
                 double *__restrict__ sums)
{
    __shared__ double red[3][256];
    const int s = blockIdx.x;
    double v[3] = {0, 0, 0};
    for (int n = cumpos[s] + threadIdx.x; n < cumpos[s + 1]; n += 256) {
        const size_t e = (size_t)arr2indx[n];
        const xh_cd z1 = F1[e], z2 = F2[e];
        const double absz1 = hypot(z1.x, z1.y), absz2 = hypot(z2.x, z2.y);
        v[0] += z1.x * z2.x + z1.y * z2.y;
        v[1] += absz1 * absz1;
        v[2] += absz2 * absz2;
    }
    xh_tree256(red, v);
    if (threadIdx.x == 0)
        for (int c = 0; c < 3; ++c) sums[3 * s + c] = red[c][0];
}

// :436-443: the cosine in float in the reference's order, the test, the weight
__device__ __forceinline__ bool fso_in_cone(float xd, float yd, float zd, float ux, float uy, float uz, float cosAngle, float aux, float &w)
{
    const float cosine = fabsf(xd * ux + yd * uy + zd * uz);
    if (!(cosine >= cosAngle)) return false;
    const float t = cosine - 1;
    w = expf(-(t * t) * aux);
    return true;
}

// :428-457 of one segment for every direction: part [segment][direction][3], pcount [segment][direction]. Lane t works for direction
// lane_dir [t]: neighbouring directions share a wave, and a wave whose cones all miss a coefficient skips the weight and the sums
__global__ void __launch_bounds__(FSO_MAX_DIR)
k_fso_cones(const float *__restrict__ fx, const float *__restrict__ fy, const float *__restrict__ fz, const float *__restrict__ rz, const float *__restrict__ a1,
            const float *__restrict__ a2, const FsoSeg *__restrict__ segs, const float *__restrict__ dirs, const int *__restrict__ lane_dir, int ndir,
            float cosAngle, float aux, double *__restrict__ part, int *__restrict__ pcount)
{
    extern __shared__ __align__(8) unsigned char fso_cone_smem[];
    FsoCoef *cf = reinterpret_cast<FsoCoef *>(fso_cone_smem);
    const FsoSeg sg = segs[blockIdx.x];
    for (int q = threadIdx.x; q < sg.len; q += blockDim.x) {
        const int n = sg.start + q;
        cf[q] = FsoCoef{fx[n], fy[n], fz[n], rz[n], a1[n], a2[n]};
    }
    __syncthreads();
    if ((int)threadIdx.x >= ndir) return;
    const int dir = lane_dir[threadIdx.x];
    const float xd = dirs[3 * dir], yd = dirs[3 * dir + 1], zd = dirs[3 * dir + 2];
    double num = 0, den1 = 0, den2 = 0;
    int cnt = 0;
    for (int q = 0; q < sg.len; ++q) {
        const FsoCoef u = cf[q];
        float w;
        if (fso_in_cone(xd, yd, zd, u.x, u.y, u.z, cosAngle, aux, w)) {
            const double wd = w;
            num += wd * (double)u.r;
            den1 += wd * (double)u.a;
            den2 += wd * (double)u.b;
            ++cnt;
        }
    }
    const size_t o = (size_t)blockIdx.x * ndir + dir;
    part[3 * o] = num; part[3 * o + 1] = den1; part[3 * o + 2] = den2;
    pcount[o] = cnt;
}

// the segments of each (shell, direction) added in increasing order: sums [direction][L][3], counts [direction][L]
__global__ void __launch_bounds__(256)
k_fso_seg_reduce(const double *__restrict__ part, const int *__restrict__ pcount, const int *__restrict__ segfirst, int L, int ndir, double *__restrict__ sums,
                 long long *__restrict__ counts)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)L * ndir) return;
    const int shell = (int)(t / ndir), dir = (int)(t - (size_t)shell * ndir);
    double num = 0, den1 = 0, den2 = 0;
    long long cnt = 0;
    for (int sg = segfirst[shell]; sg < segfirst[shell + 1]; ++sg) {
        const size_t o = (size_t)sg * ndir + dir;
        num += part[3 * o]; den1 += part[3 * o + 1]; den2 += part[3 * o + 2];
        cnt += pcount[o];
    }
    const size_t w = (size_t)dir * L + shell;
    sums[3 * w] = num; sums[3 * w + 1] = den1; sums[3 * w + 2] = den2;
    counts[w] = cnt;
}

// :496-506 and :1501-1508 for sorted coefficient n, the directions in ascending order: half [arr2indx [n]] = threeD / norm, NaN -> 1
__global__ void __launch_bounds__(256)
k_fso_threed(const float *__restrict__ fx, const float *__restrict__ fy, const float *__restrict__ fz, const int *__restrict__ freqidx,
             const int *__restrict__ arr2indx, int ncomps, const float *__restrict__ dirs, int ndir, const float *__restrict__ fsc, int L, float cosAngle, float aux,
             double *__restrict__ half)
{
    extern __shared__ float fso_dirs[];
    for (int q = threadIdx.x; q < 3 * ndir; q += 256) fso_dirs[q] = dirs[q];
    __syncthreads();
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= ncomps) return;
    const float ux = fx[n], uy = fy[n], uz = fz[n];
    const int ind = freqidx[n];
    float threeD = 0, norm = 0;
    for (int dir = 0; dir < ndir; ++dir) {
        float w;
        if (fso_in_cone(fso_dirs[3 * dir], fso_dirs[3 * dir + 1], fso_dirs[3 * dir + 2], ux, uy, uz, cosAngle, aux, w)) {
            const double wd = w;
            const double p = wd * (double)fsc[(size_t)dir * L + ind];
            threeD = (float)((double)threeD + p);
            norm = (float)((double)norm + wd);
        }
    }
    const float q = threeD / norm;
    double value = q;
    if (isnan(value)) value = 1.0;
    half[arr2indx[n]] = value;
}

// the two fixes of the empty lines (:1521-1539): column 0 takes column 1 on the rows i > Y / 2 of every plane, then on row 0 of every plane
__global__ void __launch_bounds__(256) k_fso_line_fix(double *__restrict__ half, XhDims d)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= d.Z * d.Y) return;
    const int i = t % d.Y;
    if (i > d.Y / 2 || i == 0) {
        double *row = half + (size_t)t * d.xh;
        row[0] = row[1];
    }
}

// getCompleteFourier (:1277-1293) and CenterFFT(.., true) (:1302): the completed element (k, i, j) lands at ((k + Z / 2) % Z, ..)
__global__ void __launch_bounds__(256) k_fso_full(const double *__restrict__ half, double *__restrict__ full, XhDims d)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)d.Z * d.Y * d.X) return;
    const int j = (int)(t % d.X);
    const size_t r = t / d.X;
    const int i = (int)(r % d.Y), k = (int)(r / d.Y);
    double v;
    if (j < d.xh) v = half[((size_t)k * d.Y + i) * d.xh + j];
    else v = half[((size_t)((d.Z - k) % d.Z) * d.Y + (d.Y - i) % d.Y) * d.xh + (d.X - j)];
    full[((size_t)((k + d.Z / 2) % d.Z) * d.Y + (i + d.Y / 2) % d.Y) * d.X + (j + d.X / 2) % d.X] = v;
}

// ---------------------------------------------------------------- the direction set
struct FsoVec { double x, y, z; };

FsoVec fso_unit(FsoVec v)
{
    const double n = std::sqrt(v.x * v.x + v.y * v.y + v.z * v.z);
    return FsoVec{v.x / n, v.y / n, v.z / n};
}

// an icosahedron with a vertex on +z, `level` rounds of edge-midpoint subdivision projected to the sphere; the points in level order
void fso_icosphere(int level, std::vector<FsoVec> &pts)
{
    const double PI = 3.14159265358979323846, tilt = std::atan(2.0);
    pts.clear();
    pts.push_back(FsoVec{0, 0, 1});
    for (int k = 0; k < 5; ++k) {
        const double rot = (36 + 72 * k) * PI / 180;
        pts.push_back(FsoVec{std::sin(tilt) * std::cos(rot), std::sin(tilt) * std::sin(rot), std::cos(tilt)});
    }
    for (int k = 0; k < 5; ++k) {
        const double rot = (72 * k) * PI / 180;
        pts.push_back(FsoVec{std::sin(tilt) * std::cos(rot), std::sin(tilt) * std::sin(rot), -std::cos(tilt)});
    }
    pts.push_back(FsoVec{0, 0, -1});
    // upper vertex u_k = 1 + k at rot 36 + 72 k, lower vertex l_k = 6 + k at rot 72 k: l_k lies between u_{k-1} and u_k
    std::vector<std::array<int, 3>> faces;
    for (int k = 0; k < 5; ++k) {
        const int u0 = 1 + k, u1 = 1 + (k + 1) % 5, l0 = 6 + k, l1 = 6 + (k + 1) % 5;
        faces.push_back({0, u0, u1});
        faces.push_back({u0, l1, u1});
        faces.push_back({l0, l1, u0});
        faces.push_back({11, l1, l0});
    }
    for (int round = 0; round < level; ++round) {
        std::map<std::pair<int, int>, int> mid;
        auto midpoint = [&](int a, int b) {
            const std::pair<int, int> key(std::min(a, b), std::max(a, b));
            auto it = mid.find(key);
            if (it != mid.end()) return it->second;
            pts.push_back(fso_unit(FsoVec{pts[a].x + pts[b].x, pts[a].y + pts[b].y, pts[a].z + pts[b].z}));
            return mid[key] = (int)pts.size() - 1;
        };
        std::vector<std::array<int, 3>> next;
        for (const auto &f : faces) {
            const int ab = midpoint(f[0], f[1]), bc = midpoint(f[1], f[2]), ca = midpoint(f[2], f[0]);
            next.push_back({f[0], ab, ca});
            next.push_back({f[1], bc, ab});
            next.push_back({f[2], ca, bc});
            next.push_back({ab, bc, ca});
        }
        faces.swap(next);
    }
}

double fso_round4(double v) { return std::round(v * 1e4) / 1e4; }

}  // namespace

struct xh_fso : XhVolume {
    int L = 0, seg = 0, nchunks = 0, ncomps = 0, nseg = 0;
    XhBuf F1, F2, work, counts, total, cumpos, sums, fx, fy, fz, freqidx, arr2indx, rz, a1, a2, segs, segfirst, dirs, lane_dir, part, pcount, dsums, dcounts, fsc;
    std::vector<int> hcumpos;
    XhLapTimer<FSO_NT> tm;
    bool loaded = false;
    ~xh_fso() { finish(); }
};

namespace {

int fso_check_cone(const char *who, const xh_fso *h, const float *h_dirs, int ndir, float cosAngle, float aux)
{
    XH_CHECK(h && h_dirs, XH_ERR_ARG, "%s: null argument", who);
    XH_CHECK(h->loaded, XH_ERR_STATE, "%s: nothing is loaded", who);
    XH_CHECK(ndir >= 1 && ndir <= FSO_MAX_DIR, XH_ERR_ARG, "%s: %d directions (1 .. %d)", who, ndir, FSO_MAX_DIR);
    for (int i = 0; i < 3 * ndir; ++i) XH_CHECK(std::isfinite(h_dirs[i]), XH_ERR_ARG, "%s: direction %d is not finite", who, i / 3);
    XH_CHECK(cosAngle > 0 && cosAngle < 1 && std::isfinite(aux), XH_ERR_ARG, "%s: a cone with cosine %g (the angle must lie inside (0, 90) degrees)", who, cosAngle);
    return XH_OK;
}

}  // namespace

extern "C" {

int xh_fso_directions(int32_t level, float *h_rot_tilt_deg, int32_t cap, int32_t *n)
{
    XH_CHECK(n && level >= 0 && level <= 5 && cap >= 0 && (h_rot_tilt_deg || cap == 0), XH_ERR_ARG, "xh_fso_directions: bad argument (levels 0 .. 5)");
    std::vector<FsoVec> pts, kept;
    fso_icosphere(level, pts);
    const double eps = 1e-9, PI = 3.14159265358979323846;
    for (FsoVec p : pts) {
        // one direction of every antipodal pair: the one in the upper half space; on the equator the one with y > 0 (x > 0 on the x axis)
        if (p.z < -eps || (std::fabs(p.z) <= eps && (p.y < -eps || (std::fabs(p.y) <= eps && p.x < 0)))) p = FsoVec{-p.x, -p.y, -p.z};
        bool seen = false;
        for (const FsoVec &q : kept) seen = seen || (std::fabs(p.x - q.x) + std::fabs(p.y - q.y) + std::fabs(p.z - q.z) < 1e-6);
        if (!seen) kept.push_back(p);
    }
    *n = (int32_t)kept.size();
    for (int i = 0; i < std::min<int>(cap, *n); ++i) {
        const FsoVec &p = kept[i];
        double rot = std::atan2(p.y, p.x) * 180 / PI, tilt = std::acos(std::max(-1.0, std::min(1.0, p.z))) * 180 / PI;
        if (std::fabs(p.x) <= eps && std::fabs(p.y) <= eps) rot = 0;
        rot = fso_round4(rot);
        if (rot < 0) rot += 360;
        if (rot >= 360 || rot == 0) rot = 0;      // (-0 as well)
        h_rot_tilt_deg[2 * i] = (float)rot;
        h_rot_tilt_deg[2 * i + 1] = (float)fso_round4(tilt);
    }
    return XH_OK;
}

int xh_fso_unit_vectors(const float *h_rot_tilt_deg, int32_t n, float *h_dirs)
{
    XH_CHECK(h_rot_tilt_deg && h_dirs && n >= 0, XH_ERR_ARG, "xh_fso_unit_vectors: bad argument");
    // generateDirections :985, angles *= PI / 180.0 on a Matrix2D<float>: xmippCore's operator*=(T) takes the factor as a float (that
    // header is not in this tree: SURVEY.md Appendix B, parity unpinned)
    const float deg2rad = (float)(3.14159265358979323846 / 180.0);
    for (int i = 0; i < n; ++i) {
        const float rot = h_rot_tilt_deg[2 * i] * deg2rad, tilt = h_rot_tilt_deg[2 * i + 1] * deg2rad;
        h_dirs[3 * i] = sinf(tilt) * cosf(rot);      // fscDir_fast :408-410
        h_dirs[3 * i + 1] = sinf(tilt) * sinf(rot);
        h_dirs[3 * i + 2] = cosf(tilt);
    }
    return XH_OK;
}

double xh_fso_incomplete_gamma(double x)
{
    // P(5, i / 2) = 1 - exp(-x) sum_{k < 5} x^k / k!, to 5 significant digits and then to float: the table of :526-566
    long idx = std::isnan(x) ? 0 : (long)std::max(-1.0, std::min(41.0, std::round(2 * x)));
    idx = std::max(0L, std::min(40L, idx));
    const double t = 0.5 * (double)idx;
    double term = 1, sum = 0;
    for (int k = 0; k < 5; ++k) {
        sum += term;
        term *= t / (k + 1);
    }
    const double P = 1 - std::exp(-t) * sum;
    char buf[32];
    snprintf(buf, sizeof(buf), "%.4e", P);
    return (double)(float)strtod(buf, nullptr);
}

int xh_fso_cone(double ang_con_deg, float *cosAngle, float *aux)
{
    XH_CHECK(cosAngle && aux, XH_ERR_ARG, "xh_fso_cone: null argument");
    XH_CHECK(ang_con_deg > 0 && ang_con_deg < 90, XH_ERR_ARG, "xh_fso_cone: a cone angle of %g degrees (it must lie inside (0, 90))", ang_con_deg);
    const double ang_con = ang_con_deg * 3.14159265358979323846 / 180.0;   // run :1344
    *cosAngle = (float)std::cos(ang_con);                                    // :419
    *aux = (float)(4.0 / ((*cosAngle - 1) * (*cosAngle - 1)));               // :425
    return XH_OK;
}

int xh_fso_decide(const double *h_sums, const float *h_dirs, int32_t ndir, int32_t L, int32_t xdim, double sampling, double thrs, float *h_fsc, double *h_resol,
                  float *h_fso, double *h_bingham)
{
    XH_CHECK(h_sums && h_dirs && h_fsc && h_resol && h_fso && h_bingham && ndir >= 1 && L >= 1 && xdim >= 1, XH_ERR_ARG, "xh_fso_decide: bad argument");
    std::vector<float> aniParam((size_t)L, 0.f);
    std::vector<double> freqMat((size_t)L * 9, 0.0);
    for (int k = 0; k < ndir; ++k) {
        const float x_dir = h_dirs[3 * k], y_dir = h_dirs[3 * k + 1], z_dir = h_dirs[3 * k + 2];
        const float v[3] = {x_dir, y_dir, z_dir};
        double T[9];                                                  // :413-417: float products in a double matrix
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) T[3 * a + b] = v[a] * v[b];
        bool flagRes = true;
        double resol = -1;                                            // run :1393
        for (int i = 0; i < L; ++i) {                                 // :466-486
            const double *s = h_sums + 3 * ((size_t)k * L + i);
            const double auxfsc = s[0] / (std::sqrt(s[1] * s[2]) + 1e-38);
            const float fsc = (float)std::max(0.0, auxfsc);
            h_fsc[(size_t)k * L + i] = fsc;
            if (fsc >= thrs) {
                for (int q = 0; q < 9; ++q) freqMat[9 * (size_t)i + q] += T[q];
                aniParam[i] += 1.0;                                   // anistropyParameter :989-999
            }
            if (flagRes && i > 2 && fsc <= thrs) {
                flagRes = false;
                const double ff = (float)i / (xdim * sampling);
                resol = 1. / ff;
            }
        }
        h_resol[k] = resol;
    }
    for (int i = 0; i < L; ++i) {                                     // run :1426-1464
        h_bingham[i] = 0;
        if (!(aniParam[i] > 0)) continue;
        double T[9], trT2 = 0;
        for (int q = 0; q < 9; ++q) T[q] = freqMat[9 * (size_t)i + q] / aniParam[i];
        for (int a = 0; a < 3; ++a) {
            double t2 = 0;
            for (int b = 0; b < 3; ++b) t2 += T[3 * a + b] * T[3 * b + a];
            trT2 += t2;
        }
        const double pdim = 3;
        h_bingham[i] = 0.5 * pdim * (pdim + 2) * (2 * aniParam[i]) * (trT2 - 1. / pdim);
    }
    const float nd = (float)(double)ndir;                             // :1468: a float array divided by a scalar of its type
    for (int i = 0; i < L; ++i) h_fso[i] = i < 5 ? 1.0f : aniParam[i] / nd;
    return XH_OK;
}

int xh_fso_resolution_distribution(const float *h_dirs, int32_t ndir, const double *h_resol, double ang_con_deg, double *h_out)
{
    XH_CHECK(h_dirs && h_resol && h_out && ndir >= 1, XH_ERR_ARG, "xh_fso_resolution_distribution: bad argument");
    const double PI = 3.14159265358979323846;
    const double ang_con = ang_con_deg * PI / 180.0;
    const float cosAngle = cosf(ang_con);                             // :1205-1206
    const float aux = 4.0 / ((cosAngle - 1) * (cosAngle - 1));
    for (int i = 0; i < 360; ++i) {
        const float rotmatrix = i * PI / 180.0;
        const float cr = cosf(rotmatrix), sr = sinf(rotmatrix);
        for (int j = 0; j < 91; ++j) {
            const float tiltmatrix = j * PI / 180.0;
            const float st = sinf(tiltmatrix);
            const float xx = st * cr, yy = st * sr, zz = cosf(tiltmatrix);
            double w = 0, wt = 0;
            for (int k = 0; k < ndir; ++k) {                          // x_dir, y_dir, z_dir of :1235-1237 are the unit vectors of the cones
                float cosine = fabsf(h_dirs[3 * k] * xx + h_dirs[3 * k + 1] * yy + h_dirs[3 * k + 2] * zz);
                if (cosine >= cosAngle) {
                    cosine = expf(-((cosine - 1) * (cosine - 1)) * aux);
                    w += cosine * h_resol[k];
                    wt += cosine;
                }
            }
            h_out[i * 91 + j] = w / wt;
        }
    }
    return XH_OK;
}

int xh_fso_create(xh_ctx *ctx, int32_t Z, int32_t Y, int32_t X, int32_t seg, xh_fso **out)
{
    XH_CHECK(ctx && out, XH_ERR_ARG, "xh_fso_create: null argument");
    XH_CHECK(Z >= 8 && Y >= 8 && X >= 8, XH_ERR_ARG, "xh_fso_create: a box of %d x %d x %d: sides below 8 are refused", Z, Y, X);
    XH_CHECK(Z <= 1024 && Y <= 1024 && X <= 1024, XH_ERR_UNSUPPORTED, "xh_fso_create: sizes above 1024 are not supported (%d x %d x %d)", Z, Y, X);
    XH_CHECK(!((X & 1) && (!(Y & 1) || !(Z & 1))), XH_ERR_UNSUPPORTED,
             "xh_fso_create: an odd X = %d beside an even Y or Z: a coefficient at f = 0.5 has shell X / 2 + 1, one past the shells", X);
    XH_CHECK(seg <= FSO_SEG_MAX, XH_ERR_ARG, "xh_fso_create: a segment of %d coefficients (at most %d; 0: the default)", seg, FSO_SEG_MAX);
    std::unique_ptr<xh_fso> h(new xh_fso);
    XH_TRY(h->init(ctx, Z, Y, X));
    h->L = X / 2 + 1;
    h->seg = seg > 0 ? seg : FSO_SEG_DEFAULT;
    h->nchunks = (int)((h->NF + FSO_CHUNK - 1) / FSO_CHUNK);
    XH_TRY(xh_buf_alloc(ctx, h->F1, sizeof(xh_cd) * h->NF));
    XH_TRY(xh_buf_alloc(ctx, h->F2, sizeof(xh_cd) * h->NF));
    XH_TRY(xh_buf_alloc(ctx, h->counts, sizeof(int) * (size_t)h->L * h->nchunks));
    XH_TRY(xh_buf_alloc(ctx, h->total, sizeof(int) * h->L));
    XH_TRY(xh_buf_alloc(ctx, h->cumpos, sizeof(int) * (h->L + 1)));
    XH_TRY(xh_buf_alloc(ctx, h->segfirst, sizeof(int) * (h->L + 1)));
    XH_TRY(xh_buf_alloc(ctx, h->sums, sizeof(double) * 3 * h->L));
    XH_TRY(h->tm.create(ctx));
    *out = h.release();
    return XH_OK;
}

int xh_fso_destroy(xh_fso *h)
{
    delete h;
    return XH_OK;
}

int xh_fso_load(xh_fso *h, const double *d_half1, const double *d_half2, const double *d_mask, double *h_sums, int64_t *h_shell_count, int64_t *ncomps)
{
    XH_CHECK(h && d_half1 && d_half2 && h_sums, XH_ERR_ARG, "xh_fso_load: null argument");
    XH_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    const XhDims d = h->d;
    const int L = h->L, nchunks = h->nchunks;
    h->loaded = false;
    XH_TRY(h->tm.start());
    // prepareData :1013-1024 and run :1324-1325; xmippCore's forward transform carries the 1 / N
    const double *in[2] = {d_half1, d_half2};
    xh_cd *F[2] = {(xh_cd *)h->F1.p, (xh_cd *)h->F2.p};
    if (d_mask) XH_TRY(xh_buf_reserve(h->ctx, h->work, sizeof(double) * h->N));
    const unsigned gridN = xh_grid256(h->N, h->ctx->num_cus, 4);
    for (int m = 0; m < 2; ++m) {
        if (d_mask) XH_LAUNCH256(h->ctx, k_fso_mask, gridN, in[m], d_mask, (double *)h->work.p, h->N);
        XH_TRY(h->fft.r2c(d_mask ? (const double *)h->work.p : in[m], F[m], 1.0 / (double)h->N));
    }
    XH_TRY(h->tm.lap(FSO_T_TRANSFORMS));
    // the layout: count, scan, cumpos on the host (it cuts the segments from it as well), fill
    const size_t lds = sizeof(int) * L;
    hipLaunchKernelGGL(k_fso_layout<false>, dim3(nchunks), dim3(64), lds, st, (const xh_cd *)F[0], (const xh_cd *)F[1], h->NF, d, L, nchunks, ip(h->counts), nullptr, nullptr,
                       nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    XH_LAUNCH_CHECK();
    XH_LAUNCH256(h->ctx, k_fso_scan, L, ip(h->counts), nchunks, ip(h->total));
    std::vector<int> total(L);
    XH_HIP(hipMemcpyAsync(total.data(), h->total.p, sizeof(int) * L, hipMemcpyDeviceToHost, st));
    XH_HIP(hipStreamSynchronize(st));
    h->hcumpos.assign(L + 1, 0);
    for (int s = 0; s < L; ++s) h->hcumpos[s + 1] = h->hcumpos[s] + total[s];
    h->ncomps = h->hcumpos[L];
    XH_CHECK(h->ncomps >= 1 && total[0] >= 1, XH_ERR_STATE, "xh_fso_load: the layout kept %d coefficients", h->ncomps);
    // the segments: at most seg consecutive coefficients of one shell, without sorted position 0 (the DC coefficient)
    std::vector<FsoSeg> segs;
    std::vector<int> segfirst(L + 1, 0);
    for (int s = 0; s < L; ++s) {
        segfirst[s] = (int)segs.size();
        for (int p = std::max(1, h->hcumpos[s]); p < h->hcumpos[s + 1]; p += h->seg) segs.push_back(FsoSeg{p, std::min(h->seg, h->hcumpos[s + 1] - p)});
    }
    segfirst[L] = (int)segs.size();
    h->nseg = (int)segs.size();
    XH_HIP(hipMemcpyAsync(h->cumpos.p, h->hcumpos.data(), sizeof(int) * (L + 1), hipMemcpyHostToDevice, st));
    XH_HIP(hipMemcpyAsync(h->segfirst.p, segfirst.data(), sizeof(int) * (L + 1), hipMemcpyHostToDevice, st));
    XH_TRY(xh_buf_reserve(h->ctx, h->segs, sizeof(FsoSeg) * std::max<size_t>(1, segs.size())));
    if (!segs.empty()) XH_HIP(hipMemcpyAsync(h->segs.p, segs.data(), sizeof(FsoSeg) * segs.size(), hipMemcpyHostToDevice, st));
    XH_HIP(hipStreamSynchronize(st));     // segs and segfirst are locals
    for (XhBuf *b : {&h->fx, &h->fy, &h->fz, &h->freqidx, &h->arr2indx, &h->rz, &h->a1, &h->a2}) XH_TRY(xh_buf_reserve(h->ctx, *b, 4 * (size_t)h->ncomps));
    XH_LAUNCH256(h->ctx, k_fso_add_cumpos, L, ip(h->counts), nchunks, (const int *)h->cumpos.p);
    hipLaunchKernelGGL(k_fso_layout<true>, dim3(nchunks), dim3(64), lds, st, (const xh_cd *)F[0], (const xh_cd *)F[1], h->NF, d, L, nchunks, ip(h->counts), fp(h->fx),
                       fp(h->fy), fp(h->fz), ip(h->freqidx), ip(h->arr2indx), fp(h->rz), fp(h->a1), fp(h->a2));
    XH_LAUNCH_CHECK();
    XH_LAUNCH256(h->ctx, k_fso_shell_sums, L, (const xh_cd *)F[0], (const xh_cd *)F[1], (const int *)h->arr2indx.p, (const int *)h->cumpos.p, (double *)h->sums.p);
    XH_HIP(hipMemcpyAsync(h_sums, h->sums.p, sizeof(double) * 3 * L, hipMemcpyDeviceToHost, st));
    XH_HIP(hipStreamSynchronize(st));
    XH_TRY(h->tm.lap(FSO_T_LAYOUT));
    if (h_shell_count)
        for (int s = 0; s < L; ++s) h_shell_count[s] = total[s];
    if (ncomps) *ncomps = h->ncomps;
    h->loaded = true;
    return XH_OK;
}

int xh_fso_info(const xh_fso *h, int64_t *ncomps, int32_t *nshell, int32_t *nseg, int32_t *seg)
{
    XH_CHECK(h, XH_ERR_ARG, "xh_fso_info: null handle");
    if (nshell) *nshell = h->L;
    if (seg) *seg = h->seg;
    XH_CHECK(h->loaded || (!ncomps && !nseg), XH_ERR_STATE, "xh_fso_info: nothing is loaded");
    if (ncomps) *ncomps = h->ncomps;
    if (nseg) *nseg = h->nseg;
    return XH_OK;
}

int xh_fso_layout(xh_fso *h, float *h_fx, float *h_fy, float *h_fz, int32_t *h_freqidx, int32_t *h_arr2indx, float *h_real_z1z2, float *h_absz1, float *h_absz2)
{
    XH_CHECK(h && h_fx && h_fy && h_fz && h_freqidx && h_arr2indx && h_real_z1z2 && h_absz1 && h_absz2, XH_ERR_ARG, "xh_fso_layout: null argument");
    XH_CHECK(h->loaded, XH_ERR_STATE, "xh_fso_layout: nothing is loaded");
    XH_HIP(hipSetDevice(h->ctx->device));
    XH_HIP(hipStreamSynchronize(h->ctx->stream));
    const size_t bytes = 4 * (size_t)h->ncomps;
    void *dst[8] = {h_fx, h_fy, h_fz, h_freqidx, h_arr2indx, h_real_z1z2, h_absz1, h_absz2};
    XhBuf *src[8] = {&h->fx, &h->fy, &h->fz, &h->freqidx, &h->arr2indx, &h->rz, &h->a1, &h->a2};
    for (int a = 0; a < 8; ++a) XH_HIP(hipMemcpy(dst[a], src[a]->p, bytes, hipMemcpyDeviceToHost));
    return XH_OK;
}

int xh_fso_directional(xh_fso *h, const float *h_dirs, int32_t ndir, float cosAngle, float aux, double *h_sums, int64_t *h_count)
{
    XH_TRY(fso_check_cone("xh_fso_directional", h, h_dirs, ndir, cosAngle, aux));
    XH_CHECK(h_sums && h_count, XH_ERR_ARG, "xh_fso_directional: null argument");
    XH_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    const int L = h->L, nseg = h->nseg;
    const size_t pairs = (size_t)std::max(1, nseg) * ndir, cells = (size_t)L * ndir;
    XH_TRY(xh_buf_reserve(h->ctx, h->dirs, sizeof(float) * 3 * ndir));
    XH_TRY(xh_buf_reserve(h->ctx, h->part, sizeof(double) * 3 * pairs));
    XH_TRY(xh_buf_reserve(h->ctx, h->pcount, sizeof(int) * pairs));
    XH_TRY(xh_buf_reserve(h->ctx, h->dsums, sizeof(double) * 3 * cells));
    XH_TRY(xh_buf_reserve(h->ctx, h->dcounts, sizeof(long long) * cells));
    XH_HIP(hipMemcpyAsync(h->dirs.p, h_dirs, sizeof(float) * 3 * ndir, hipMemcpyHostToDevice, st));
    // spatially compact tiles of 64 directions: the 64 nearest the z axis, then the others by azimuth. Consecutive sorted coefficients point
    // the same way, so whole waves skip most of them (tools/bench_fso.py: the stage 1.04 -> 0.83 ms at 256^3). Every (segment, direction)
    // is still one lane's sum in the order of the segment: the bytes do not depend on the tiles
    std::vector<int> lane_dir(ndir);
    for (int i = 0; i < ndir; ++i) lane_dir[i] = i;
    std::stable_sort(lane_dir.begin(), lane_dir.end(), [&](int a, int b) { return std::fabs(h_dirs[3 * a + 2]) > std::fabs(h_dirs[3 * b + 2]); });
    if (ndir > 64)
        std::stable_sort(lane_dir.begin() + 64, lane_dir.end(), [&](int a, int b) {
            const float sa = h_dirs[3 * a + 2] < 0 ? -1.f : 1.f, sb = h_dirs[3 * b + 2] < 0 ? -1.f : 1.f;      // (a direction stands for its antipode too)
            return std::atan2(sa * h_dirs[3 * a + 1], sa * h_dirs[3 * a]) < std::atan2(sb * h_dirs[3 * b + 1], sb * h_dirs[3 * b]);
        });
    XH_TRY(xh_buf_reserve(h->ctx, h->lane_dir, sizeof(int) * ndir));
    XH_HIP(hipMemcpyAsync(h->lane_dir.p, lane_dir.data(), sizeof(int) * ndir, hipMemcpyHostToDevice, st));
    XH_TRY(h->tm.start());
    if (nseg > 0) {
        const int threads = 64 * ((ndir + 63) / 64);
        hipLaunchKernelGGL(k_fso_cones, dim3(nseg), dim3(threads), sizeof(FsoCoef) * h->seg, st, (const float *)h->fx.p, (const float *)h->fy.p, (const float *)h->fz.p,
                           (const float *)h->rz.p, (const float *)h->a1.p, (const float *)h->a2.p, (const FsoSeg *)h->segs.p, (const float *)h->dirs.p, (const int *)h->lane_dir.p, ndir,
                           cosAngle, aux, (double *)h->part.p, ip(h->pcount));
        XH_LAUNCH_CHECK();
    }
    XH_TRY(h->tm.lap(FSO_T_CONES));
    XH_LAUNCH256(h->ctx, k_fso_seg_reduce, (unsigned)((cells + 255) / 256), (const double *)h->part.p, (const int *)h->pcount.p, (const int *)h->segfirst.p, L, ndir,
                 (double *)h->dsums.p, (long long *)h->dcounts.p);
    std::vector<long long> counts(cells);
    XH_HIP(hipMemcpyAsync(h_sums, h->dsums.p, sizeof(double) * 3 * cells, hipMemcpyDeviceToHost, st));
    XH_HIP(hipMemcpyAsync(counts.data(), h->dcounts.p, sizeof(long long) * cells, hipMemcpyDeviceToHost, st));
    XH_HIP(hipStreamSynchronize(st));
    XH_TRY(h->tm.lap(FSO_T_SEGREDUCE));
    for (int dir = 0; dir < ndir; ++dir) {
        int64_t c = 0;
        for (int s = 0; s < L; ++s) c += counts[(size_t)dir * L + s];
        h_count[dir] = c;
    }
    return XH_OK;
}

int xh_fso_threedfsc(xh_fso *h, const float *h_dirs, int32_t ndir, float cosAngle, float aux, const float *h_fsc, double *d_half, double *d_full)
{
    XH_TRY(fso_check_cone("xh_fso_threedfsc", h, h_dirs, ndir, cosAngle, aux));
    XH_CHECK(h_fsc && d_half, XH_ERR_ARG, "xh_fso_threedfsc: null argument");
    const XhDims d = h->d;
    XH_CHECK(d.Z == d.Y && d.Y == d.X, XH_ERR_UNSUPPORTED, "xh_fso_threedfsc: the 3DFSC needs a cubic box, this one is %d x %d x %d", d.Z, d.Y, d.X);
    XH_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    const int L = h->L;
    XH_TRY(xh_buf_reserve(h->ctx, h->dirs, sizeof(float) * 3 * ndir));
    XH_TRY(xh_buf_reserve(h->ctx, h->fsc, sizeof(float) * (size_t)ndir * L));
    XH_HIP(hipMemcpyAsync(h->dirs.p, h_dirs, sizeof(float) * 3 * ndir, hipMemcpyHostToDevice, st));
    XH_HIP(hipMemcpyAsync(h->fsc.p, h_fsc, sizeof(float) * (size_t)ndir * L, hipMemcpyHostToDevice, st));
    XH_TRY(h->tm.start());
    XH_HIP(hipMemsetAsync(d_half, 0, sizeof(double) * h->NF, st));
    hipLaunchKernelGGL(k_fso_threed, dim3((unsigned)((h->ncomps + 255) / 256)), dim3(256), sizeof(float) * 3 * ndir, st, (const float *)h->fx.p, (const float *)h->fy.p,
                       (const float *)h->fz.p, (const int *)h->freqidx.p, (const int *)h->arr2indx.p, h->ncomps, (const float *)h->dirs.p, ndir, (const float *)h->fsc.p, L,
                       cosAngle, aux, d_half);
    XH_LAUNCH_CHECK();
    XH_LAUNCH256(h->ctx, k_fso_line_fix, (unsigned)((d.Z * d.Y + 255) / 256), d_half, d);
    if (d_full) XH_LAUNCH256(h->ctx, k_fso_full, (unsigned)((h->N + 255) / 256), (const double *)d_half, d_full, d);
    XH_HIP(hipStreamSynchronize(st));     // the host arrays were copied from
    XH_TRY(h->tm.lap(FSO_T_3DFSC));
    return XH_OK;
}

int xh_fso_set_timing(xh_fso *h, int32_t on)
{
    XH_CHECK(h, XH_ERR_ARG, "xh_fso_set_timing: null handle");
    h->tm.set(on != 0);
    return XH_OK;
}

int xh_fso_stage_ms(const xh_fso *h, double *h_ms)
{
    XH_CHECK(h && h_ms, XH_ERR_ARG, "xh_fso_stage_ms: null argument");
    h->tm.read(h_ms);
    return XH_OK;
}

}  // extern "C"
