// Host tables of the curved / over-integrated sw2d solver, from the caller's descriptor alone: validation, index maps,
// straight-element compression, the face structure of the nodal-trace form, tile order, operator images. Plain host
// arithmetic, no HIP: sw2d_curved_device.hip uploads what build() returns, bdg_sw2d_curved_plan reports its decisions.
#pragma once
#include "blitzdg_hip.h"
#include <vector>

namespace blitzdg {
namespace curved_tables {

// What the tables need of an order's kernel table (CurvedKernelTable), asked for the descriptor's sizes.
struct KernelSizes {
    int Np = 0, KV = 0, MT = 0;
    int opsTiles = 0, opsOff[8] = {};   // general image: offVc, offDrT, offDsT, offIT, offM, offMF, offF, offGI
    bool ntFits = false;                // the nodal-trace image fits its kernel's LDS plan
    int ntTiles = 0, ntOff[5] = {};     // nodal-trace image: VCH, SCH, KE, offSurf(0), offMass
};

// The creation-time switches (BDG_SW2D_CURVED_GENERAL, _NO_AFFINE, _NO_TILE_ORDER), read by the caller.
struct Switches {
    bool general = false, noAffine = false, noTileOrder = false;
};

// How straight an element is, from the tables themselves (to 1e-10 relative: the tables of a fine mesh carry that much
// round-off from Dr x). kCubStraight: rx, ry, sx, sy do not vary over the cubature points. kStraight: the nodal Jacobian
// and the face normals at the Gauss points are constant as well.
enum Straightness : char { kNotStraight = 0, kCubStraight = 1, kStraight = 2 };

struct Tables {
    int N = 0, Np = 0, K = 0, ncub = 0, ncb = 0, ng = 0, fb = 0;
    long long ld = 0, sideLd = 0;        // K and the curved count rounded up to 64
    // index maps: flat Gauss id -> padded row * ld + element, walls as -(offset + 1); offM only when gmapM is rewired
    bool identityM = true;
    std::vector<int> offP, offM;         // (48 fb, K); dropped again on the nodal-trace form, which has no trace planes
    std::vector<int> maxNeighbour;       // largest element a face of element k is paired with
    std::vector<int> curved, slotOf;     // set(curvedEls) in the caller's order; ld slots, -1: not listed
    // general form: straight elements hold 4 numbers c with (W rx, W ry, W sx, W sy)[i] = wref[i] * c
    int kref = -1, numAffine = 0;        // reference element: the first cubature-straight one, listed or not
    std::vector<int> affineEl;           // ld flags
    std::vector<double> cubAffine, wref; // (4, K); 16 ncb weights of kref
    // nodal-trace form (useNT): face nodes, neighbours' nodes, wall / straight flags, 14 numbers per straight element
    bool useNT = false;
    int krefNT = -1, numAffineNT = 0, rowsP = 0; // reference element: the first fully straight one outside curvedEls
    std::vector<int> nodeP, faceFlags, faceNodes, tileOrder; // (rowsP, K); ld; rowsP; tiles (empty: mesh order)
    std::vector<double> elAffine, wrefNT, gaussWref;         // (14, K); 16 ncb weights of krefNT; 16 fb half Gauss weights
    // operator images in MFMA A-tile order, inverse mass matrices of the listed elements (Np, Np per slot)
    std::vector<double> ops, opsNT, minv;
    double bytesPerElement = 0.0;
};

// Argument checks that need no table: sizes, required pointers, the wall and curved lists.
void validate(const bdg_sw2d_curved_desc& d);

// Everything above. Throws bdg_detail::arg_error with the texts of bdg_sw2d_curved_create.
Tables build(const bdg_sw2d_curved_desc& d, const KernelSizes& ks, const Switches& sw);

// One plane of the device tables into out (rows, K): W * (rx, ry, sx, sy)[g] at the cubature points, and 1 / J.
void weightedGeometry(const bdg_sw2d_curved_desc& d, int g, std::vector<double>& out);
void inverseJacobian(const bdg_sw2d_curved_desc& d, int Np, std::vector<double>& out);

// Compulsory bytes of one RHS evaluation per element, on the form the tables chose.
double bytesPerElement(const bdg_sw2d_curved_desc& d, const Tables& t);

} // namespace curved_tables
} // namespace blitzdg
