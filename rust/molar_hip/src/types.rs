//! `#[repr(C)]` mirrors of the types of `include/molar_hip.h` (line numbers refer to that header).

use std::os::raw::c_void;

/// Opaque engine context (`molar_hip_ctx`, header :62): one HIP stream plus engine-owned device buffers.
#[repr(C)]
pub struct MolarHipCtx {
    _opaque: [u8; 0],
}

/// Opaque XTC reader (`molar_hip_xtc`).
#[repr(C)]
pub struct MolarHipXtc {
    _opaque: [u8; 0],
}

/// Opaque streamed fit (`molar_hip_fit_stream`): per-frame Kabsch fit of host-memory frames, selection packed by host threads.
#[repr(C)]
pub struct MolarHipFitStream {
    _opaque: [u8; 0],
}

/// `molar_hip_box` (header :96-101): MolAR's `PeriodicBox` (periodic_box.rs:15-23) - matrix with columns a, b, c,
/// its inverse and the triclinic correction shifts.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct MolarHipBox {
    pub m: [f32; 9],
    pub inv: [f32; 9],
    pub nshift: i32,
    pub shifts: [f32; 78],
}

/// `molar_hip_search_desc` (header :137-155): one distance-search request.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct MolarHipSearchDesc {
    pub kind: i32,
    pub cutoff: f32,
    pub xyz1: *const f32,
    pub natoms1: usize,
    pub idx1: *const u64,
    pub n1: usize,
    pub xyz2: *const f32,
    pub natoms2: usize,
    pub idx2: *const u64,
    pub n2: usize,
    pub vdw1: *const f32,
    pub vdw2: *const f32,
    pub ids_local: i32,
    pub box9: *const f32,
    pub pbc: u8,
    pub lower3: *const f32,
    pub upper3: *const f32,
}

impl Default for MolarHipSearchDesc {
    fn default() -> Self {
        // all-zero is the C side's "unset" for every field
        unsafe { std::mem::zeroed() }
    }
}

/// `molar_hip_contact_groups`: group labels of the contact-count calls, one per SELECTED atom of each set.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct MolarHipContactGroups {
    pub group1: *const u32,
    pub ngroups1: usize,
    pub group2: *const u32,
    pub ngroups2: usize,
}

impl Default for MolarHipContactGroups {
    fn default() -> Self {
        unsafe { std::mem::zeroed() }
    }
}

/// `molar_hip_density_grid`: the grid of the density calls - `mode` (0: BOX, fractional coordinates of each frame's box; 1: LAB,
/// the range `lo .. hi`), the bins per dimension (1 integrates over it), and the mask of the dimensions that are centred.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct MolarHipDensityGrid {
    pub mode: u32,
    pub nbins: [u32; 3],
    pub lo: [f64; 3],
    pub hi: [f64; 3],
    pub centre_dims: u32,
}

/// `MolarHipDensityGrid::mode`
pub const DENSITY_BOX: u32 = 0;
pub const DENSITY_LAB: u32 = 1;

/// `molar_hip_intcoord_spec`: what the internal-coordinate calls compute - `kind` (the atoms per tuple: 2 distance, 3 angle,
/// 4 dihedral), the bins of the histogram and of the map per side (0: none), and the half-open range of a distance histogram.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct MolarHipIntcoordSpec {
    pub kind: u32,
    pub nbins: u32,
    pub map_bins: u32,
    pub reserved: u32,
    pub lo: f64,
    pub hi: f64,
}

/// `MolarHipIntcoordSpec::kind`
pub const IC_DISTANCE: u32 = 2;
pub const IC_ANGLE: u32 = 3;
pub const IC_DIHEDRAL: u32 = 4;

/// `molar_hip_tcf_spec`: what the time correlation calls compute - `kind` (the atoms per tuple: 1 the atom's own 3-vector,
/// 2 the bond vector, 3 the plane normal), `mode` (TCF_UNIT: unit vectors, TCF_RAW: the vectors as they are) and `dims` (the
/// bits x, y, z of the components that enter, 1 ..= 7).
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct MolarHipTcfSpec {
    pub kind: u32,
    pub mode: u32,
    pub dims: u32,
    pub reserved: u32,
}

/// `MolarHipTcfSpec::mode`
pub const TCF_UNIT: u32 = 0;
pub const TCF_RAW: u32 = 1;

/// `molar_hip_sfactor_grid`: the reciprocal lattice of the structure factor calls - the largest Miller indices (H, K, L): h in
/// 0 ..= H, k in -K ..= K, l in -L ..= L - and `nshells` shells of |q| of width `dq` from `qmin` (0: no shells).
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct MolarHipSfactorGrid {
    pub hmax: [u32; 3],
    pub qmin: f64,
    pub dq: f64,
    pub nshells: u32,
    pub reserved: u32,
}

/// `molar_hip_mindist_spec`: the request of the minimum-distance calls - the PbcDims mask, whether set 2 is set 1 (`same`) and
/// whether pairs inside one group are skipped then, the frames walked at once (0: chosen by the call) and the cutoff of the
/// contact frequency map.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct MolarHipMindistSpec {
    pub pbc: u32,
    pub same: u32,
    pub exclude_same_group: u32,
    pub frame_block: u32,
    pub cutoff: f64,
}
pub const MINDIST_DIST: u32 = 1;
pub const MINDIST_ATOM1: u32 = 2;
pub const MINDIST_ATOM2: u32 = 4;
pub const MINDIST_MAT: u32 = 8;

/// `MOLAR_HIP_VANHOVE_SIGNED`: the one component of `dims` itself instead of the length of the displacement.
pub const VANHOVE_SIGNED: u32 = 1;

/// The parameters of `Engine::van_hove` (molar_hip_vanhove; the definition: molar_hip.h): the half-open range [lo, hi) and its
/// bins, the stride of the time origins, the bits x, y, z of the components that enter, and `VANHOVE_SIGNED` or 0.
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct VanHoveSpec {
    pub lo: f64,
    pub hi: f64,
    pub nbins: usize,
    pub origin_stride: usize,
    pub dims: u32,
    pub flags: u32,
}

/// What `Engine::van_hove` returns: hist [group][lag][bin], outside [group][lag] (the pairs beyond the range), norigins [lag],
/// nvalid [group] (the particles that entered), bad [selected particle] (its frames with a coordinate that is not finite) and
/// the nbins + 1 bin edges.  For every (g, l): the sum of hist over the bins plus outside equals nvalid[g] * norigins[l].
#[derive(Debug, Clone, Default)]
pub struct VanHove {
    pub hist: Vec<u64>,
    pub outside: Vec<u64>,
    pub norigins: Vec<u64>,
    pub nvalid: Vec<u64>,
    pub bad: Vec<u32>,
    pub edges: Vec<f64>,
    pub ngroups: usize,
    pub nlags: usize,
    pub nbins: usize,
}

/// What `Engine::van_hove_plan` returns (molar_hip_vanhove_plan): the device workspace and every launch-shape size the kernels
/// branch on.
#[derive(Debug, Clone, Copy, Default, PartialEq)]
pub struct VanHovePlan {
    pub workspace_bytes: usize,
    pub particles_per_wg: u32,
    pub origins_per_pass: u32,
    pub lag_tile: u32,
    pub on_chip: u32,
    pub lds_cells: u32,
    pub pass_splits: u32,
    pub pairs_per_flush: u64,
}

/// `molar_hip_search_desc_f64`: the same request for MolAR built with its `f64` feature (Float = f64).
#[repr(C)]
#[derive(Clone, Copy)]
pub struct MolarHipSearchDescF64 {
    pub kind: i32,
    pub cutoff: f64,
    pub xyz1: *const f64,
    pub natoms1: usize,
    pub idx1: *const u64,
    pub n1: usize,
    pub xyz2: *const f64,
    pub natoms2: usize,
    pub idx2: *const u64,
    pub n2: usize,
    pub vdw1: *const f64,
    pub vdw2: *const f64,
    pub ids_local: i32,
    pub box9: *const f64,
    pub pbc: u8,
    pub lower3: *const f64,
    pub upper3: *const f64,
}

impl Default for MolarHipSearchDescF64 {
    fn default() -> Self {
        unsafe { std::mem::zeroed() }
    }
}

/// `molar_hip_membrane_patches`: CSR of the patch (neighbour) lists of K lipids.
#[repr(C)]
pub struct MolarHipMembranePatches {
    pub nlipids: usize,
    pub patch_offsets: *const u64,
    pub patch_ids: *const u64,
}

/// `molar_hip_membrane_state`: per-lipid arrays updated by one smoothing pass (molar_membrane/src/lib.rs:661-812).
#[repr(C)]
pub struct MolarHipMembraneState {
    pub head_markers: *mut f32,
    pub normals: *mut f32,
    pub valid: *mut u8,
    pub quad_coefs: *mut f32,
    pub mean_curv: *mut f32,
    pub gauss_curv: *mut f32,
    pub princ_curvs: *mut f32,
    pub princ_dirs: *mut f32,
    pub area: *mut f32,
    pub nvert: *mut u32,
    pub neib_ids: *mut u64,
    pub voro_vertexes: *mut f32,
    pub fitted_patch_points: *mut f32,
}

/// `molar_hip_membrane_state_f64`: the same arrays in f64, for molar_membrane built with its `f64` feature.
#[repr(C)]
pub struct MolarHipMembraneStateF64 {
    pub head_markers: *mut f64,
    pub normals: *mut f64,
    pub valid: *mut u8,
    pub quad_coefs: *mut f64,
    pub mean_curv: *mut f64,
    pub gauss_curv: *mut f64,
    pub princ_curvs: *mut f64,
    pub princ_dirs: *mut f64,
    pub area: *mut f64,
    pub nvert: *mut u32,
    pub neib_ids: *mut u64,
    pub voro_vertexes: *mut f64,
    pub fitted_patch_points: *mut f64,
}

/// `molar_hip_membrane_plan`: opaque handle of the chained bilayer frame call (molar_hip_membrane_frame_*).
#[repr(C)]
pub struct MolarHipMembranePlan {
    _private: [u8; 0],
}

/// `molar_hip_membrane_desc`: what is constant over a trajectory - index lists (host memory, copied at creation) and the
/// options of Membrane::compute the chained call covers (molar_membrane/src/lib.rs:53-85, 410-454).
#[repr(C)]
pub struct MolarHipMembraneDesc {
    pub natoms: usize,
    pub nlipids: usize,
    pub lipid_idx: *const u64,
    pub lipid_offsets: *const u64,
    pub marker_idx: *const u64,
    pub marker_offsets: *const u64,
    pub masses: *const f32,
    pub ntails: usize,
    pub tail_idx: *const u64,
    pub tail_offsets: *const u64,
    pub tail_lipid: *const u32,
    pub tail_bonds: *const u8,
    pub cutoff: f32,
    pub order_type: i32,
    pub max_smooth_iter: i32,
    pub unwrap: i32,
    pub use_global_normal: i32,
    pub global_normal: [f32; 3],
}

/// `molar_hip_membrane_view`: device addresses and sizes of one frame's results.
#[repr(C)]
pub struct MolarHipMembraneView {
    pub nlipids: usize,
    pub patch_entries: usize,
    pub npairs: usize,
    pub head: *const f32,
    pub mid: *const f32,
    pub tail: *const f32,
    pub patch_offsets: *const u64,
    pub patch_ids: *const u64,
    pub initial_normals: *const f32,
    pub valid: *const u8,
    pub smoothed_head: *const f32,
    pub normals: *const f32,
    pub quad_coefs: *const f32,
    pub mean_curv: *const f32,
    pub gauss_curv: *const f32,
    pub princ_curvs: *const f32,
    pub princ_dirs: *const f32,
    pub area: *const f32,
    pub nvert: *const u32,
    pub neib_ids: *const u64,
    pub voro_vertexes: *const f32,
    pub fitted_patch_points: *const f32,
    pub order: *const f32,
    pub norder: usize,
}

/// `molar_hip_membrane_out`: host destinations of `molar_hip_membrane_frame_fetch` (null = skip).
#[repr(C)]
pub struct MolarHipMembraneOut {
    pub head: *mut f32,
    pub mid: *mut f32,
    pub tail: *mut f32,
    pub patch_offsets: *mut u64,
    pub patch_ids: *mut u64,
    pub initial_normals: *mut f32,
    pub valid: *mut u8,
    pub smoothed_head: *mut f32,
    pub normals: *mut f32,
    pub quad_coefs: *mut f32,
    pub mean_curv: *mut f32,
    pub gauss_curv: *mut f32,
    pub princ_curvs: *mut f32,
    pub princ_dirs: *mut f32,
    pub area: *mut f32,
    pub nvert: *mut u32,
    pub neib_ids: *mut u64,
    pub voro_vertexes: *mut f32,
    pub fitted_patch_points: *mut f32,
    pub order: *mut f32,
}

/// Search kinds (header :124-129) = the four driver families of distance_search.rs.
pub const SEARCH_SINGLE: i32 = 0;
pub const SEARCH_DOUBLE: i32 = 1;
pub const SEARCH_WITHIN: i32 = 2;
pub const SEARCH_DOUBLE_VDW: i32 = 3;

/// `PbcDims` bit masks (periodic_box.rs:126-128).
pub const PBC_FULL: u8 = 7;
pub const PBC_NONE: u8 = 0;

/// A raw `hipStream_t` handed to `molar_hip_set_stream`.
pub type HipStream = *mut c_void;
