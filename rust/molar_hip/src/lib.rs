//! Host shim between MolAR and the MI355X engine (`libmolar_hip.so`).
//!
//! **Source only**: this crate has not been compiled in the repository's build image (no `cargo` / `rustc` there).
//! `src/ffi.rs` is generated from `include/molar_hip.h` by `tools/gen_rust_ffi.py`, and
//! `tests/test_rust_shim_cpu.py` asserts that the symbol set, the argument counts and the safe wrappers below stay in
//! step with the C header.
//!
//! What MolAR hands over is exactly what its provider traits already hold:
//!
//! | MolAR                                                   | this crate                         |
//! |---------------------------------------------------------|------------------------------------|
//! | `PosProvider::coords_ptr()` (providers.rs:96-106)       | `&[[f32; 3]]`, the WHOLE frame     |
//! | `IndexSliceProvider::get_index_slice()` (:45-76)        | `Option<&[usize]>` (None = all)    |
//! | `AtomStorage::masses()` (atom_storage.rs:272)           | `&[f32]`, full-length column       |
//! | `PeriodicBox` matrix, columns a,b,c (periodic_box.rs)   | `&[f32; 9]` column-major           |
//! | `PbcDims` (periodic_box.rs:70-128)                      | `u8` mask                          |
//!
//! Loading follows MolAR's own plugin crate (molar_gromacs/src/lib.rs:95-176): `MOLAR_HIP_PLUGIN` at run time, then
//! the path baked in at compile time, then the system search path; symbols are resolved once into a table of function
//! pointers; the loaded plugin is cached process-wide.  When no library (or no GPU) is found the caller keeps MolAR's
//! CPU path - `Engine::try_default()` returns `None`, nothing else changes.

pub mod ffi;
pub mod types;

use std::ffi::CStr;
use std::sync::{Arc, OnceLock};

use ffi::MolarHipFns;
pub use types::*;

/// MolAR's `Float` (molar/src/aliases.rs:10-13).
#[cfg(not(feature = "f64"))]
pub type Float = f32;
#[cfg(feature = "f64")]
pub type Float = f64;

/// Errors of the engine, mapped from the C status codes (header :38-55) onto MolAR's error enums.
#[derive(thiserror::Error, Debug)]
pub enum EngineError {
    #[error("engine library not available: {0}")]
    Load(#[from] libloading::Error),
    /// `MeasureError::Sizes` (measure.rs:732-762)
    #[error("incompatible sizes: {0}")]
    Sizes(String),
    /// `MeasureError::ZeroMass`
    #[error("zero mass")]
    ZeroMass,
    /// `MeasureError::Svd`
    #[error("SVD failed")]
    Svd,
    /// `MeasureError::NoPbc`
    #[error("pbc operation without periodic box")]
    NoPbc,
    /// `PeriodicBoxError` (periodic_box.rs:131-144)
    #[error("periodic box: {0}")]
    PeriodicBox(String),
    /// `LipidOrderError` (measure.rs:281-291)
    #[error("lipid order: {0}")]
    LipidOrder(String),
    #[error("engine: {0}")]
    Other(String),
}

/// The loaded library plus its resolved entry points.  The `Library` must outlive every call through the table, which
/// holding both in one struct guarantees.
pub struct Plugin {
    _lib: libloading::Library,
    pub fns: MolarHipFns,
}

// The table is plain function pointers; contexts are what must not be shared between threads (see `Engine`).
unsafe impl Send for Plugin {}
unsafe impl Sync for Plugin {}

impl Plugin {
    fn open_library() -> Result<libloading::Library, libloading::Error> {
        // 1. user override at run time
        if let Ok(path) = std::env::var("MOLAR_HIP_PLUGIN") {
            return unsafe { libloading::Library::new(path) };
        }
        // 2. location recorded when the crate was built
        if let Some(path) = option_env!("MOLAR_HIP_PLUGIN") {
            if let Ok(lib) = unsafe { libloading::Library::new(path) } {
                return Ok(lib);
            }
        }
        // 3. system search path
        unsafe { libloading::Library::new(libloading::library_filename("molar_hip")) }
    }

    pub fn load() -> Result<Self, libloading::Error> {
        let lib = Self::open_library()?;
        let fns = unsafe { MolarHipFns::resolve(&lib)? };
        Ok(Plugin { _lib: lib, fns })
    }

    /// Process-wide instance; loaded at most once, a failed attempt is retried by the next call.
    pub fn get_cached() -> Result<Arc<Self>, libloading::Error> {
        static CACHE: OnceLock<Arc<Plugin>> = OnceLock::new();
        if let Some(p) = CACHE.get() {
            return Ok(Arc::clone(p));
        }
        let fresh = Arc::new(Self::load()?);
        let _ = CACHE.set(Arc::clone(&fresh));
        Ok(CACHE.get().map(Arc::clone).unwrap_or(fresh))
    }

    fn last_error(&self) -> String {
        unsafe {
            let p = (self.fns.last_error)();
            if p.is_null() { String::new() } else { CStr::from_ptr(p).to_string_lossy().into_owned() }
        }
    }

    fn check(&self, status: i32) -> Result<(), EngineError> {
        match status {
            0 => Ok(()),
            1 => Err(EngineError::Sizes(self.last_error())),
            2 => Err(EngineError::ZeroMass),
            3 => Err(EngineError::Svd),
            4 => Err(EngineError::NoPbc),
            5 | 6 | 10 => Err(EngineError::PeriodicBox(self.last_error())),
            7..=9 => Err(EngineError::LipidOrder(self.last_error())),
            _ => Err(EngineError::Other(self.last_error())),
        }
    }
}

/// One engine context = one HIP stream with its device buffers.  Not `Sync`: MolAR calls `Measure` from rayon workers
/// on disjoint selections (system.rs:193-213) - give each worker its own `Engine`, or use the `*_batch` calls.
pub struct Engine {
    plugin: Arc<Plugin>,
    ctx: *mut MolarHipCtx,
}

unsafe impl Send for Engine {}

impl Drop for Engine {
    fn drop(&mut self) {
        unsafe { (self.plugin.fns.destroy)(self.ctx) }
    }
}

/// What `Engine::sasa` and `Engine::sasa_vol` return: the reference's `Sasa` (sasa.rs:82-97), per selected atom in selection
/// order; `volumes` is empty and `total_volume` 0 after `sasa`.
#[derive(Debug, Clone)]
pub struct Sasa {
    pub areas: Vec<f32>,
    pub total_area: f64,
    pub volumes: Vec<f32>,
    pub total_volume: f64,
}

fn idx_ptr(idx: Option<&[usize]>) -> (*const u64, usize) {
    // usize == u64 on every target MolAR supports (aliases.rs); the engine reads u64
    match idx {
        Some(s) => (s.as_ptr() as *const u64, s.len()),
        None => (std::ptr::null(), 0),
    }
}

// The C ABI trusts its pointer/size pairs.  Safe callers cannot be allowed to hand it a mass column shorter than the
// frame, an index past the end of the coordinates or a CSR split that leaves its index slice: the wrappers below check
// exactly what the engine will dereference and return `EngineError::Sizes` instead of reading out of bounds.
fn check_index(index: Option<&[usize]>, natoms: usize, what: &str) -> Result<(), EngineError> {
    if let Some(ix) = index {
        if let Some(&bad) = ix.iter().find(|&&a| a >= natoms) {
            return Err(EngineError::Sizes(format!("{what}: index {bad} is out of range for {natoms} atoms")));
        }
    }
    Ok(())
}

// Contact counts: the engine adds into `deg*` at every selected position and into `map` at every pair of labels, so the
// slices must cover exactly that (labels2 None: a single-set request, the map is ngroups1 x ngroups1).
#[allow(clippy::too_many_arguments)]
fn check_contact_outputs(
    what: &str, nsel1: usize, deg1: Option<&[u64]>, labels1: Option<(&[u32], usize)>, labels2: Option<(&[u32], usize)>, nsel2: usize,
    deg2: Option<&[u64]>, map: Option<&[u64]>,
) -> Result<Option<MolarHipContactGroups>, EngineError> {
    if deg1.is_some_and(|d| d.len() != nsel1) || deg2.is_some_and(|d| d.len() != nsel2) {
        return Err(EngineError::Sizes(format!("{what}: a degree array must have one entry per selected atom")));
    }
    let Some((l1, g1)) = labels1 else {
        if map.is_some() {
            return Err(EngineError::Sizes(format!("{what}: a map needs labels")));
        }
        return Ok(None);
    };
    let (l2, g2) = labels2.unwrap_or((l1, g1));
    if l1.len() != nsel1 || (labels2.is_some() && l2.len() != nsel2) {
        return Err(EngineError::Sizes(format!("{what}: one label per selected atom is needed")));
    }
    if l1.iter().any(|&l| l as usize >= g1) || l2.iter().any(|&l| l as usize >= g2) {
        return Err(EngineError::Sizes(format!("{what}: a label is not below the number of groups")));
    }
    if map.is_some_and(|m| Some(m.len()) != g1.checked_mul(g2)) {
        return Err(EngineError::Sizes(format!("{what}: the map must have ngroups1 x ngroups2 = {g1} x {g2} entries")));
    }
    Ok(Some(MolarHipContactGroups {
        group1: l1.as_ptr(), ngroups1: g1, group2: if labels2.is_some() { l2.as_ptr() } else { std::ptr::null() }, ngroups2: if labels2.is_some() { g2 } else { 0 },
    }))
}

fn check_column(len: usize, natoms: usize, what: &str) -> Result<(), EngineError> {
    // per-atom columns (masses) are gathered through the index: they must cover the whole frame
    if len < natoms {
        return Err(EngineError::Sizes(format!("{what}: column of {len} entries for {natoms} atoms")));
    }
    Ok(())
}

fn check_offsets(offsets: &[usize], index_len: usize, what: &str) -> Result<(), EngineError> {
    if offsets.windows(2).any(|w| w[0] > w[1]) || offsets.last().map_or(false, |&e| e > index_len) {
        return Err(EngineError::Sizes(format!("{what}: offsets must be non-decreasing and end within the {index_len} indices")));
    }
    Ok(())
}

fn box_ptr(b: Option<&[f32; 9]>) -> *const f32 {
    b.map_or(std::ptr::null(), |m| m.as_ptr())
}

impl Engine {
    pub fn new(device: i32) -> Result<Self, EngineError> {
        let plugin = Plugin::get_cached()?;
        let ctx = unsafe { (plugin.fns.create)(device) };
        if ctx.is_null() {
            return Err(EngineError::Other(plugin.last_error()));
        }
        Ok(Engine { plugin, ctx })
    }

    /// `Some(engine)` on a machine with the library and a GPU, `None` otherwise: the caller stays on MolAR's CPU path.
    pub fn try_default() -> Option<Self> {
        Self::new(0).ok()
    }

    pub fn synchronize(&self) -> Result<(), EngineError> {
        self.plugin.check(unsafe { (self.plugin.fns.synchronize)(self.ctx) })
    }

    // ---------------------------------------------------------------- distance search (distance_search.rs:519-954)

    fn search(&self, d: &MolarHipSearchDesc) -> Result<Vec<(usize, usize, Float)>, EngineError> {
        let f = &self.plugin.fns;
        let mut n = 0u64;
        self.plugin.check(unsafe { (f.search_count)(self.ctx, d, &mut n) })?;
        let n = n as usize;
        let (mut i, mut j, mut dist) = (vec![0u64; n], vec![0u64; n], vec![0f32; n]);
        self.plugin.check(unsafe { (f.search_fill_usize)(self.ctx, i.as_mut_ptr(), j.as_mut_ptr(), dist.as_mut_ptr()) })?;
        Ok((0..n).map(|k| (i[k] as usize, j[k] as usize, dist[k] as Float)).collect())
    }

    /// `distance_search_single_pbc` (distance_search.rs:928-954); `box9 = None` is `distance_search_single` (:892-926).
    /// Result order is the reference's: plan order, then i-major / j-minor.
    pub fn distance_search_single(
        &self, cutoff: f32, coords: &[[f32; 3]], index: Option<&[usize]>, box9: Option<&[f32; 9]>, pbc: u8,
    ) -> Result<Vec<(usize, usize, Float)>, EngineError> {
        check_index(index, coords.len(), "distance_search_single")?;
        let (ip, n) = idx_ptr(index);
        let d = MolarHipSearchDesc {
            kind: SEARCH_SINGLE, cutoff, xyz1: coords.as_ptr() as *const f32, natoms1: coords.len(), idx1: ip, n1: n,
            box9: box_ptr(box9), pbc, ..Default::default()
        };
        self.search(&d)
    }

    /// `distance_search_double(_pbc)` (:659-754): pairs (atom of set 1, atom of set 2).
    pub fn distance_search_double(
        &self, cutoff: f32, coords1: &[[f32; 3]], index1: Option<&[usize]>, coords2: &[[f32; 3]], index2: Option<&[usize]>,
        box9: Option<&[f32; 9]>, pbc: u8,
    ) -> Result<Vec<(usize, usize, Float)>, EngineError> {
        check_index(index1, coords1.len(), "distance_search_double (set 1)")?;
        check_index(index2, coords2.len(), "distance_search_double (set 2)")?;
        let (i1, n1) = idx_ptr(index1);
        let (i2, n2) = idx_ptr(index2);
        let d = MolarHipSearchDesc {
            kind: SEARCH_DOUBLE, cutoff, xyz1: coords1.as_ptr() as *const f32, natoms1: coords1.len(), idx1: i1, n1,
            xyz2: coords2.as_ptr() as *const f32, natoms2: coords2.len(), idx2: i2, n2, box9: box_ptr(box9), pbc,
            ..Default::default()
        };
        self.search(&d)
    }

    /// `distance_search_within_pbc` (:519-598): ids of set-1 atoms within `cutoff` of set 2, duplicates as the reference
    /// emits them (the caller sorts and de-duplicates, selection_expr.rs:112).
    pub fn distance_search_within_pbc(
        &self, cutoff: f32, coords1: &[[f32; 3]], index1: Option<&[usize]>, coords2: &[[f32; 3]], index2: Option<&[usize]>,
        box9: &[f32; 9], pbc: u8,
    ) -> Result<Vec<usize>, EngineError> {
        check_index(index1, coords1.len(), "distance_search_within_pbc (set 1)")?;
        check_index(index2, coords2.len(), "distance_search_within_pbc (set 2)")?;
        let (i1, n1) = idx_ptr(index1);
        let (i2, n2) = idx_ptr(index2);
        let d = MolarHipSearchDesc {
            kind: SEARCH_WITHIN, cutoff, xyz1: coords1.as_ptr() as *const f32, natoms1: coords1.len(), idx1: i1, n1,
            xyz2: coords2.as_ptr() as *const f32, natoms2: coords2.len(), idx2: i2, n2, box9: box9.as_ptr(), pbc,
            ..Default::default()
        };
        let f = &self.plugin.fns;
        let mut n = 0u64;
        self.plugin.check(unsafe { (f.search_count)(self.ctx, &d, &mut n) })?;
        let mut ids = vec![0u64; n as usize];
        self.plugin.check(unsafe { (f.search_fill_ids)(self.ctx, ids.as_mut_ptr()) })?;
        Ok(ids.into_iter().map(|v| v as usize).collect())
    }

    /// `within <cutoff> pbc of <inner>` as the selection keeps it (`LogicalNode::Within`, selection/ast.rs:589-631): what
    /// `SortedSet::from_unsorted` (selection_expr.rs:112) makes of the stream above - sorted, de-duplicated - computed
    /// without the stream: an atom stops looking at its first hit in any plan entry (molar_hip_within_count / _fill).
    pub fn within_set_pbc(
        &self, cutoff: f32, coords1: &[[f32; 3]], index1: Option<&[usize]>, coords2: &[[f32; 3]], index2: Option<&[usize]>,
        box9: &[f32; 9], pbc: u8,
    ) -> Result<Vec<usize>, EngineError> {
        check_index(index1, coords1.len(), "within_set_pbc (set 1)")?;
        check_index(index2, coords2.len(), "within_set_pbc (set 2)")?;
        let (i1, n1) = idx_ptr(index1);
        let (i2, n2) = idx_ptr(index2);
        let d = MolarHipSearchDesc {
            kind: SEARCH_WITHIN, cutoff, xyz1: coords1.as_ptr() as *const f32, natoms1: coords1.len(), idx1: i1, n1,
            xyz2: coords2.as_ptr() as *const f32, natoms2: coords2.len(), idx2: i2, n2, box9: box9.as_ptr(), pbc,
            ..Default::default()
        };
        let f = &self.plugin.fns;
        let mut n = 0u64;
        self.plugin.check(unsafe { (f.within_count)(self.ctx, &d, &mut n) })?;
        let mut ids = vec![0u64; n as usize];
        if n > 0 {
            self.plugin.check(unsafe { (f.within_fill)(self.ctx, ids.as_mut_ptr()) })?;
        }
        Ok(ids.into_iter().map(|v| v as usize).collect())
    }

    /// While a caller holds `&State` the first set of its `within` requests cannot change: with the hold on, consecutive
    /// `within_set_pbc` calls that name the same first set (same slices, same box) and come to the same grid reuse its staged
    /// coordinates and its grid (molar_hip_within_hold; the reference's within_size_bench.rs asks 1600 times against one frame).
    pub fn within_hold(&self, on: bool) -> Result<(), EngineError> {
        self.plugin.check(unsafe { (self.plugin.fns.within_hold)(self.ctx, if on { 1 } else { 0 }) })
    }

    /// `SearchConnectivity::from_iter(distance_search_single_pbc(..))` (connectivity.rs:19-35, modify.rs:77-78) built on the
    /// device: adjacency lists in the reference's push order as CSR over local ids (`offsets[len + 1]`, `neigh[2 * pairs]`).
    pub fn search_connectivity_pbc(
        &self, cutoff: f32, coords: &[[f32; 3]], index: Option<&[usize]>, box9: &[f32; 9], pbc: u8,
    ) -> Result<(Vec<usize>, Vec<usize>), EngineError> {
        check_index(index, coords.len(), "search_connectivity_pbc")?;
        let (ip, n) = idx_ptr(index);
        let d = MolarHipSearchDesc {
            kind: SEARCH_SINGLE, cutoff, xyz1: coords.as_ptr() as *const f32, natoms1: coords.len(), idx1: ip, n1: n,
            ids_local: 1, box9: box9.as_ptr(), pbc, ..Default::default()
        };
        let f = &self.plugin.fns;
        let (mut rows, mut entries) = (0u64, 0u64);
        self.plugin.check(unsafe { (f.search_connectivity)(self.ctx, &d, &mut rows, &mut entries) })?;
        let mut off = vec![0u64; rows as usize + 1];
        let mut nb = vec![0u64; entries as usize];
        self.plugin.check(unsafe { (f.search_connectivity_fill)(self.ctx, off.as_mut_ptr(), if entries > 0 { nb.as_mut_ptr() } else { std::ptr::null_mut() }) })?;
        Ok((off.into_iter().map(|v| v as usize).collect(), nb.into_iter().map(|v| v as usize).collect()))
    }

    // ---------------------------------------------------------------- Measure (measure.rs:22-649)

    /// `Measure::center_of_mass` (:60-75)
    pub fn center_of_mass(&self, coords: &[[f32; 3]], index: Option<&[usize]>, masses: &[f32]) -> Result<[f32; 3], EngineError> {
        check_index(index, coords.len(), "center_of_mass")?;
        check_column(masses.len(), coords.len(), "center_of_mass: masses")?;
        let (ip, n) = idx_ptr(index);
        let mut out = [0f32; 3];
        self.plugin.check(unsafe {
            (self.plugin.fns.center_of_mass)(self.ctx, coords.as_ptr() as *const f32, coords.len(), ip, n, masses.as_ptr(), out.as_mut_ptr())
        })?;
        Ok(out)
    }

    /// `Measure::sasa` (:427) through molar_hip_sasa: Shrake-Rupley areas over `npoints` points per atom, radii `vdw + probe`;
    /// `vdw` holds one radius per SELECTED atom in selection order.  `volumes` stays empty.
    pub fn sasa(&self, coords: &[[f32; 3]], index: Option<&[usize]>, vdw: &[f32], probe: f32, npoints: u32) -> Result<Sasa, EngineError> {
        self.sasa_call("sasa", coords, index, vdw, probe, npoints, false)
    }

    /// `Measure::sasa_vol` (:435; `Sasa::volumes / total_volume`, sasa.rs:92,97) through molar_hip_sasa_vol: the areas of
    /// `sasa` and the volume of each ball inside its power cell.
    pub fn sasa_vol(&self, coords: &[[f32; 3]], index: Option<&[usize]>, vdw: &[f32], probe: f32, npoints: u32) -> Result<Sasa, EngineError> {
        self.sasa_call("sasa_vol", coords, index, vdw, probe, npoints, true)
    }

    #[allow(clippy::too_many_arguments)]
    fn sasa_call(
        &self, what: &str, coords: &[[f32; 3]], index: Option<&[usize]>, vdw: &[f32], probe: f32, npoints: u32, with_volumes: bool,
    ) -> Result<Sasa, EngineError> {
        check_index(index, coords.len(), what)?;
        let (ip, n) = idx_ptr(index);
        let nsel = if index.is_some() { n } else { coords.len() };
        if vdw.len() != nsel {
            return Err(EngineError::Sizes(format!("{what}: {} radii for {nsel} selected atoms", vdw.len())));
        }
        let mut out = Sasa { areas: vec![0f32; nsel], total_area: 0.0, volumes: vec![0f32; if with_volumes { nsel } else { 0 }], total_volume: 0.0 };
        if index.is_none() && nsel == 0 {
            return Ok(out); // to the C call, no index and n == 0 would mean "all atoms"
        }
        let xyz = coords.as_ptr() as *const f32;
        if with_volumes {
            self.plugin.check(unsafe {
                (self.plugin.fns.sasa_vol)(self.ctx, xyz, coords.len(), ip, nsel, vdw.as_ptr(), probe, npoints, out.areas.as_mut_ptr(),
                                           std::ptr::null_mut(), &mut out.total_area, out.volumes.as_mut_ptr(), &mut out.total_volume)
            })?;
        } else {
            self.plugin.check(unsafe {
                (self.plugin.fns.sasa)(self.ctx, xyz, coords.len(), ip, nsel, vdw.as_ptr(), probe, npoints, out.areas.as_mut_ptr(),
                                       std::ptr::null_mut(), &mut out.total_area)
            })?;
        }
        Ok(out)
    }

    /// `Measure::gyration` (:78-87) / `gyration_pbc` (:222-232) with a box
    pub fn gyration(&self, coords: &[[f32; 3]], index: Option<&[usize]>, masses: &[f32], box9: Option<&[f32; 9]>) -> Result<f32, EngineError> {
        check_index(index, coords.len(), "gyration")?;
        check_column(masses.len(), coords.len(), "gyration: masses")?;
        let (ip, n) = idx_ptr(index);
        let mut out = 0f32;
        self.plugin.check(unsafe {
            (self.plugin.fns.gyration)(self.ctx, coords.as_ptr() as *const f32, coords.len(), ip, n, masses.as_ptr(), box_ptr(box9), &mut out)
        })?;
        Ok(out)
    }

    /// `rmsd` (:485-504)
    pub fn rmsd(&self, c1: &[[f32; 3]], i1: Option<&[usize]>, c2: &[[f32; 3]], i2: Option<&[usize]>) -> Result<f32, EngineError> {
        check_index(i1, c1.len(), "rmsd (selection 1)")?;
        check_index(i2, c2.len(), "rmsd (selection 2)")?;
        let (p1, n1) = idx_ptr(i1);
        let (p2, n2) = idx_ptr(i2);
        let mut out = 0f32;
        self.plugin.check(unsafe {
            (self.plugin.fns.rmsd)(self.ctx, c1.as_ptr() as *const f32, c1.len(), p1, n1, c2.as_ptr() as *const f32, c2.len(), p2, n2, &mut out)
        })?;
        Ok(out)
    }

    /// `fit_transform` (:507-522): (R column-major, t) with p -> R p + t moving selection 1 onto selection 2.
    pub fn fit_transform(
        &self, c1: &[[f32; 3]], i1: Option<&[usize]>, m1: &[f32], c2: &[[f32; 3]], i2: Option<&[usize]>, m2: &[f32],
    ) -> Result<([f32; 9], [f32; 3]), EngineError> {
        check_index(i1, c1.len(), "fit_transform (selection 1)")?;
        check_index(i2, c2.len(), "fit_transform (selection 2)")?;
        check_column(m1.len(), c1.len(), "fit_transform: masses 1")?;
        check_column(m2.len(), c2.len(), "fit_transform: masses 2")?;
        let (p1, n1) = idx_ptr(i1);
        let (p2, n2) = idx_ptr(i2);
        let (mut r, mut t) = ([0f32; 9], [0f32; 3]);
        self.plugin.check(unsafe {
            (self.plugin.fns.fit_transform)(self.ctx, c1.as_ptr() as *const f32, c1.len(), p1, n1, m1.as_ptr(),
                                            c2.as_ptr() as *const f32, c2.len(), p2, n2, m2.as_ptr(), 0, r.as_mut_ptr(), t.as_mut_ptr())
        })?;
        Ok((r, t))
    }

    /// `Modify::apply_transform` (modify.rs:32-36), in place
    pub fn apply_transform(&self, coords: &mut [[f32; 3]], index: Option<&[usize]>, r: &[f32; 9], t: &[f32; 3]) -> Result<(), EngineError> {
        check_index(index, coords.len(), "apply_transform")?;
        let (ip, n) = idx_ptr(index);
        self.plugin.check(unsafe {
            (self.plugin.fns.apply_transform)(self.ctx, coords.as_mut_ptr() as *mut f32, coords.len(), ip, n, r.as_ptr(), t.as_ptr())
        })
    }

    // ---- MolAR built with `f64` (Float = f64): the Measure / Modify methods on double-precision data
    // (header: "MolAR built with its `f64` feature"); the periodic ones are bound in ffi.rs.  The f64 search
    // is wrapped below as far as MolAR's own callers use it: the fused histogram, `within` as a set, SearchConnectivity and
    // unwrap_connectivity (the raw f64 drivers are bound in ffi.rs).

    /// `Measure::center_of_mass` (:60-75), f64
    pub fn center_of_mass_f64(&self, coords: &[[f64; 3]], index: Option<&[usize]>, masses: &[f64]) -> Result<[f64; 3], EngineError> {
        check_index(index, coords.len(), "center_of_mass_f64")?;
        check_column(masses.len(), coords.len(), "center_of_mass_f64: masses")?;
        let (ip, n) = idx_ptr(index);
        let mut out = [0f64; 3];
        self.plugin.check(unsafe {
            (self.plugin.fns.center_of_mass_f64)(self.ctx, coords.as_ptr() as *const f64, coords.len(), ip, n, masses.as_ptr(), out.as_mut_ptr())
        })?;
        Ok(out)
    }

    /// `Measure::gyration` (:78-87), f64
    pub fn gyration_f64(&self, coords: &[[f64; 3]], index: Option<&[usize]>, masses: &[f64]) -> Result<f64, EngineError> {
        check_index(index, coords.len(), "gyration_f64")?;
        check_column(masses.len(), coords.len(), "gyration_f64: masses")?;
        let (ip, n) = idx_ptr(index);
        let mut out = 0f64;
        self.plugin.check(unsafe {
            (self.plugin.fns.gyration_f64)(self.ctx, coords.as_ptr() as *const f64, coords.len(), ip, n, masses.as_ptr(), &mut out)
        })?;
        Ok(out)
    }

    /// `rmsd` (:485-504), f64
    pub fn rmsd_f64(&self, c1: &[[f64; 3]], i1: Option<&[usize]>, c2: &[[f64; 3]], i2: Option<&[usize]>) -> Result<f64, EngineError> {
        check_index(i1, c1.len(), "rmsd_f64 (selection 1)")?;
        check_index(i2, c2.len(), "rmsd_f64 (selection 2)")?;
        let (p1, n1) = idx_ptr(i1);
        let (p2, n2) = idx_ptr(i2);
        let mut out = 0f64;
        self.plugin.check(unsafe {
            (self.plugin.fns.rmsd_f64)(self.ctx, c1.as_ptr() as *const f64, c1.len(), p1, n1, c2.as_ptr() as *const f64, c2.len(), p2, n2, &mut out)
        })?;
        Ok(out)
    }

    /// `fit_transform` (:507-522), f64: (R column-major, t)
    pub fn fit_transform_f64(
        &self, c1: &[[f64; 3]], i1: Option<&[usize]>, m1: &[f64], c2: &[[f64; 3]], i2: Option<&[usize]>, m2: &[f64],
    ) -> Result<([f64; 9], [f64; 3]), EngineError> {
        check_index(i1, c1.len(), "fit_transform_f64 (selection 1)")?;
        check_index(i2, c2.len(), "fit_transform_f64 (selection 2)")?;
        check_column(m1.len(), c1.len(), "fit_transform_f64: masses 1")?;
        check_column(m2.len(), c2.len(), "fit_transform_f64: masses 2")?;
        let (p1, n1) = idx_ptr(i1);
        let (p2, n2) = idx_ptr(i2);
        let (mut r, mut t) = ([0f64; 9], [0f64; 3]);
        self.plugin.check(unsafe {
            (self.plugin.fns.fit_transform_f64)(self.ctx, c1.as_ptr() as *const f64, c1.len(), p1, n1, m1.as_ptr(),
                                                c2.as_ptr() as *const f64, c2.len(), p2, n2, m2.as_ptr(), 0, r.as_mut_ptr(), t.as_mut_ptr())
        })?;
        Ok((r, t))
    }

    /// `Modify::apply_transform` (modify.rs:32-36), f64, in place
    pub fn apply_transform_f64(&self, coords: &mut [[f64; 3]], index: Option<&[usize]>, r: &[f64; 9], t: &[f64; 3]) -> Result<(), EngineError> {
        check_index(index, coords.len(), "apply_transform_f64")?;
        let (ip, n) = idx_ptr(index);
        self.plugin.check(unsafe {
            (self.plugin.fns.apply_transform_f64)(self.ctx, coords.as_mut_ptr() as *mut f64, coords.len(), ip, n, r.as_ptr(), t.as_ptr())
        })
    }

    /// Contact counts of `distance_search_single(_pbc)` (f32) without the list (`molar_hip_search_contacts`): `deg[p]` += the
    /// entries with selected atom `p` (a position in the selection) as either member, and, with `labels` (one per selected
    /// atom, each below `ngroups`), `map[min(g_a, g_b) * ngroups + max(g_a, g_b)]` += 1 per entry (a, b).  Both are added
    /// into; the counts include the reference list's duplicates (header).  Returns the number of entries.
    pub fn contacts_single(
        &self, cutoff: f32, coords: &[[f32; 3]], index: Option<&[usize]>, box9: Option<&[f32; 9]>, pbc: u8, deg: Option<&mut [u64]>,
        labels: Option<(&[u32], usize)>, map: Option<&mut [u64]>,
    ) -> Result<u64, EngineError> {
        check_index(index, coords.len(), "contacts_single")?;
        let (ip, n) = idx_ptr(index);
        let nsel = if index.is_some() { n } else { coords.len() };
        let g = check_contact_outputs("contacts_single", nsel, deg.as_deref(), labels, None, 0, None, map.as_deref())?;
        let d = MolarHipSearchDesc {
            kind: SEARCH_SINGLE, cutoff, xyz1: coords.as_ptr() as *const f32, natoms1: coords.len(), idx1: ip, n1: n,
            box9: box9.map_or(std::ptr::null(), |m| m.as_ptr()), pbc, ..Default::default()
        };
        let mut count = 0u64;
        self.plugin.check(unsafe {
            (self.plugin.fns.search_contacts)(self.ctx, &d, g.as_ref().map_or(std::ptr::null(), |g| g as *const MolarHipContactGroups),
                                              deg.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr()), std::ptr::null_mut(),
                                              map.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr()), &mut count)
        })?;
        Ok(count)
    }

    /// The same for `distance_search_double(_pbc)`: `deg1[p]` += entries with first member `p`, `deg2[p]` += entries with
    /// second member `p`, `map[g1_a * ngroups2 + g2_b]` += 1.
    pub fn contacts_double(
        &self, cutoff: f32, coords1: &[[f32; 3]], index1: Option<&[usize]>, coords2: &[[f32; 3]], index2: Option<&[usize]>,
        box9: Option<&[f32; 9]>, pbc: u8, deg1: Option<&mut [u64]>, deg2: Option<&mut [u64]>, labels1: Option<(&[u32], usize)>,
        labels2: Option<(&[u32], usize)>, map: Option<&mut [u64]>,
    ) -> Result<u64, EngineError> {
        check_index(index1, coords1.len(), "contacts_double (set 1)")?;
        check_index(index2, coords2.len(), "contacts_double (set 2)")?;
        let (i1, n1) = idx_ptr(index1);
        let (i2, n2) = idx_ptr(index2);
        let nsel1 = if index1.is_some() { n1 } else { coords1.len() };
        let nsel2 = if index2.is_some() { n2 } else { coords2.len() };
        if labels1.is_some() != labels2.is_some() {
            return Err(EngineError::Sizes("contacts_double: labels are needed for both sets or for none".into()));
        }
        let g = check_contact_outputs("contacts_double", nsel1, deg1.as_deref(), labels1, labels2, nsel2, deg2.as_deref(), map.as_deref())?;
        let d = MolarHipSearchDesc {
            kind: SEARCH_DOUBLE, cutoff, xyz1: coords1.as_ptr() as *const f32, natoms1: coords1.len(), idx1: i1, n1,
            xyz2: coords2.as_ptr() as *const f32, natoms2: coords2.len(), idx2: i2, n2,
            box9: box9.map_or(std::ptr::null(), |m| m.as_ptr()), pbc, ..Default::default()
        };
        let mut count = 0u64;
        self.plugin.check(unsafe {
            (self.plugin.fns.search_contacts)(self.ctx, &d, g.as_ref().map_or(std::ptr::null(), |g| g as *const MolarHipContactGroups),
                                              deg1.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr()), deg2.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr()),
                                              map.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr()), &mut count)
        })?;
        Ok(count)
    }

    /// Connected components of the contact graph of `distance_search_single(_pbc)` (f32) without the list
    /// (`molar_hip_search_clusters`): the particles are the selected atoms (positions in the selection) or, with `labels` (one
    /// per selected atom, each below `ngroups`), the groups.  Returns `(comp_of, sizes)`: the component of every particle, and
    /// the particles per component; components are numbered in the order of their smallest particle, so the pieces of a
    /// selection (`split_mol_iter` taken by distance) are the runs of equal `comp_of`.
    pub fn clusters(
        &self, cutoff: f32, coords: &[[f32; 3]], index: Option<&[usize]>, box9: Option<&[f32; 9]>, pbc: u8, labels: Option<(&[u32], usize)>,
    ) -> Result<(Vec<u32>, Vec<u32>), EngineError> {
        check_index(index, coords.len(), "clusters")?;
        let (ip, n) = idx_ptr(index);
        let nsel = if index.is_some() { n } else { coords.len() };
        let g = check_contact_outputs("clusters", nsel, None, labels, None, 0, None, None)?;
        let np = labels.map_or(nsel, |(_, ng)| ng);
        let d = MolarHipSearchDesc {
            kind: SEARCH_SINGLE, cutoff, xyz1: coords.as_ptr() as *const f32, natoms1: coords.len(), idx1: ip, n1: n,
            box9: box9.map_or(std::ptr::null(), |m| m.as_ptr()), pbc, ..Default::default()
        };
        let (mut comp_of, mut sizes, mut ncomp) = (vec![0u32; np], vec![0u32; np], 0u32);
        self.plugin.check(unsafe {
            (self.plugin.fns.search_clusters)(self.ctx, &d, g.as_ref().map_or(std::ptr::null(), |g| g as *const MolarHipContactGroups),
                                              comp_of.as_mut_ptr(), sizes.as_mut_ptr(), std::ptr::null_mut(), std::ptr::null_mut(), &mut ncomp)
        })?;
        sizes.truncate(ncomp as usize);
        Ok((comp_of, sizes))
    }

    /// Hydrogen bonds of one frame (`molar_hip_hbonds_counts` + `molar_hip_hbonds_fill`; the definition is in the header):
    /// donors `index1` and acceptors `index2` of ONE frame `coords`, the donors' hydrogens as a CSR over the donors
    /// (`h_offsets[ndonors + 1]`, `h_idx`: atom indices).  `angle_kind` 0: angle(D-H-A) >= `angle_deg`; 1: angle(H-D-A) <=
    /// `angle_deg`; `max_ha` > 0 adds |H-A| <= `max_ha`.  `don_count[p]` / `acc_count[q]` += the bonds of the donor / acceptor at
    /// that position, `map[g1 * ngroups2 + g2]` += 1.  Returns the sorted triples (donor, hydrogen, acceptor) and, per triple,
    /// (|D-A|, |H-A|, the angle in degrees).
    pub fn hbonds(
        &self, cutoff: f32, coords: &[[f32; 3]], index1: Option<&[usize]>, h_offsets: &[usize], h_idx: &[usize], index2: Option<&[usize]>,
        box9: Option<&[f32; 9]>, pbc: u8, angle_kind: i32, angle_deg: f64, max_ha: f64, don_count: Option<&mut [u64]>,
        acc_count: Option<&mut [u64]>, labels1: Option<(&[u32], usize)>, labels2: Option<(&[u32], usize)>, map: Option<&mut [u64]>,
    ) -> Result<(Vec<[u32; 3]>, Vec<[f64; 3]>), EngineError> {
        check_index(index1, coords.len(), "hbonds (donors)")?;
        check_index(index2, coords.len(), "hbonds (acceptors)")?;
        check_index(Some(h_idx), coords.len(), "hbonds (hydrogens)")?;
        let (i1, n1) = idx_ptr(index1);
        let (i2, n2) = idx_ptr(index2);
        let nsel1 = if index1.is_some() { n1 } else { coords.len() };
        let nsel2 = if index2.is_some() { n2 } else { coords.len() };
        if h_offsets.len() != nsel1 + 1 || h_offsets[0] != 0 || h_offsets[nsel1] != h_idx.len() || h_offsets.windows(2).any(|w| w[1] < w[0]) {
            return Err(EngineError::Sizes("hbonds: h_offsets must run from 0 to h_idx.len() over ndonors + 1 entries without decreasing".into()));
        }
        if labels1.is_some() != labels2.is_some() {
            return Err(EngineError::Sizes("hbonds: labels are needed for both sets or for none".into()));
        }
        let g = check_contact_outputs("hbonds", nsel1, don_count.as_deref(), labels1, labels2, nsel2, acc_count.as_deref(), map.as_deref())?;
        let d = MolarHipSearchDesc {
            kind: SEARCH_DOUBLE, cutoff, xyz1: coords.as_ptr() as *const f32, natoms1: coords.len(), idx1: i1, n1,
            xyz2: coords.as_ptr() as *const f32, natoms2: coords.len(), idx2: i2, n2,
            box9: box9.map_or(std::ptr::null(), |m| m.as_ptr()), pbc, ..Default::default()
        };
        let mut count = 0u64;
        self.plugin.check(unsafe {
            (self.plugin.fns.hbonds_counts)(self.ctx, &d, h_offsets.as_ptr() as *const u64, h_idx.as_ptr() as *const u64, h_idx.len(), angle_kind,
                                            angle_deg, max_ha, g.as_ref().map_or(std::ptr::null(), |g| g as *const MolarHipContactGroups),
                                            don_count.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr()),
                                            acc_count.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr()),
                                            map.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr()), &mut count)
        })?;
        let n = count as usize;
        let mut triples = vec![[0u32; 3]; n];
        let (mut da, mut ha, mut ang) = (vec![0f64; n], vec![0f64; n], vec![0f64; n]);
        if n > 0 {
            self.plugin.check(unsafe {
                (self.plugin.fns.hbonds_fill)(self.ctx, triples.as_mut_ptr() as *mut u32, da.as_mut_ptr(), ha.as_mut_ptr(), ang.as_mut_ptr())
            })?;
        }
        Ok((triples, (0..n).map(|k| [da[k], ha[k], ang[k]]).collect()))
    }

    /// The fused radial distance histogram in f64: the pairs of `distance_search_single(_pbc)` with Float = f64, each
    /// distance through the f64 `Histogram1D::add_one` (molar_membrane/src/stats.rs:29-35) over `bins.len()` bins of
    /// [hmin, hmax), added into `bins`; no pair list.  Returns the number of pairs within the cutoff (binned or not).
    pub fn histogram_single_f64(
        &self, cutoff: f64, coords: &[[f64; 3]], index: Option<&[usize]>, box9: Option<&[f64; 9]>, pbc: u8, hmin: f64, hmax: f64,
        bins: &mut [u64],
    ) -> Result<u64, EngineError> {
        check_index(index, coords.len(), "histogram_single_f64")?;
        let (ip, n) = idx_ptr(index);
        let d = MolarHipSearchDescF64 {
            kind: SEARCH_SINGLE, cutoff, xyz1: coords.as_ptr() as *const f64, natoms1: coords.len(), idx1: ip, n1: n,
            box9: box9.map_or(std::ptr::null(), |m| m.as_ptr()), pbc, ..Default::default()
        };
        let mut count = 0u64;
        self.plugin.check(unsafe {
            (self.plugin.fns.search_histogram_f64)(self.ctx, &d, hmin, hmax, bins.len(), bins.as_mut_ptr(), &mut count)
        })?;
        Ok(count)
    }

    /// The same for `distance_search_double(_pbc)` with Float = f64: pairs (atom of set 1, atom of set 2).
    pub fn histogram_double_f64(
        &self, cutoff: f64, coords1: &[[f64; 3]], index1: Option<&[usize]>, coords2: &[[f64; 3]], index2: Option<&[usize]>,
        box9: Option<&[f64; 9]>, pbc: u8, hmin: f64, hmax: f64, bins: &mut [u64],
    ) -> Result<u64, EngineError> {
        check_index(index1, coords1.len(), "histogram_double_f64 (set 1)")?;
        check_index(index2, coords2.len(), "histogram_double_f64 (set 2)")?;
        let (i1, n1) = idx_ptr(index1);
        let (i2, n2) = idx_ptr(index2);
        let d = MolarHipSearchDescF64 {
            kind: SEARCH_DOUBLE, cutoff, xyz1: coords1.as_ptr() as *const f64, natoms1: coords1.len(), idx1: i1, n1,
            xyz2: coords2.as_ptr() as *const f64, natoms2: coords2.len(), idx2: i2, n2,
            box9: box9.map_or(std::ptr::null(), |m| m.as_ptr()), pbc, ..Default::default()
        };
        let mut count = 0u64;
        self.plugin.check(unsafe {
            (self.plugin.fns.search_histogram_f64)(self.ctx, &d, hmin, hmax, bins.len(), bins.as_mut_ptr(), &mut count)
        })?;
        Ok(count)
    }

    /// The exact bin edges of the f64 histogram over the squared distance (host arithmetic, no GPU): `nbins + 1` values,
    /// edges[b] = the smallest d2 >= 0 whose bin is >= b.
    pub fn histogram_edges_f64(&self, hmin: f64, hmax: f64, nbins: usize) -> Result<Vec<f64>, EngineError> {
        let mut e = vec![0f64; nbins + 1];
        self.plugin.check(unsafe { (self.plugin.fns.histogram_edges_f64)(hmin, hmax, nbins, e.as_mut_ptr()) })?;
        Ok(e)
    }

    /// `within <cutoff> [pbc] of <inner>` with Float = f64 as the selection keeps it: `SortedSet::from_unsorted` of the f64
    /// stream, computed without the stream (molar_hip_within_count_f64 / _fill_f64).  `box9` = None: the non-periodic form,
    /// which needs `bounds` = (lower, upper) as `distance_search_within` does.
    pub fn within_set_f64(
        &self, cutoff: f64, coords1: &[[f64; 3]], index1: Option<&[usize]>, coords2: &[[f64; 3]], index2: Option<&[usize]>,
        box9: Option<&[f64; 9]>, pbc: u8, bounds: Option<(&[f64; 3], &[f64; 3])>,
    ) -> Result<Vec<usize>, EngineError> {
        check_index(index1, coords1.len(), "within_set_f64 (set 1)")?;
        check_index(index2, coords2.len(), "within_set_f64 (set 2)")?;
        let (i1, n1) = idx_ptr(index1);
        let (i2, n2) = idx_ptr(index2);
        let d = MolarHipSearchDescF64 {
            kind: SEARCH_WITHIN, cutoff, xyz1: coords1.as_ptr() as *const f64, natoms1: coords1.len(), idx1: i1, n1,
            xyz2: coords2.as_ptr() as *const f64, natoms2: coords2.len(), idx2: i2, n2,
            box9: box9.map_or(std::ptr::null(), |m| m.as_ptr()), pbc,
            lower3: bounds.map_or(std::ptr::null(), |b| b.0.as_ptr()), upper3: bounds.map_or(std::ptr::null(), |b| b.1.as_ptr()),
            ..Default::default()
        };
        let f = &self.plugin.fns;
        let mut n = 0u64;
        self.plugin.check(unsafe { (f.within_count_f64)(self.ctx, &d, &mut n) })?;
        let mut ids = vec![0u64; n as usize];
        if n > 0 {
            self.plugin.check(unsafe { (f.within_fill_f64)(self.ctx, ids.as_mut_ptr()) })?;
        }
        Ok(ids.into_iter().map(|v| v as usize).collect())
    }

    /// `SearchConnectivity::from_iter(distance_search_single(_pbc)(..))` with Float = f64, built on the device: adjacency lists
    /// in the reference's push order as CSR over local ids (`offsets[len + 1]`, `neigh[2 * pairs]`).  The CSR is u64 in both
    /// precisions: the fill call is the f32 form's.
    pub fn search_connectivity_f64(
        &self, cutoff: f64, coords: &[[f64; 3]], index: Option<&[usize]>, box9: Option<&[f64; 9]>, pbc: u8,
    ) -> Result<(Vec<usize>, Vec<usize>), EngineError> {
        check_index(index, coords.len(), "search_connectivity_f64")?;
        let (ip, n) = idx_ptr(index);
        let d = MolarHipSearchDescF64 {
            kind: SEARCH_SINGLE, cutoff, xyz1: coords.as_ptr() as *const f64, natoms1: coords.len(), idx1: ip, n1: n,
            ids_local: 1, box9: box9.map_or(std::ptr::null(), |m| m.as_ptr()), pbc, ..Default::default()
        };
        let f = &self.plugin.fns;
        let (mut rows, mut entries) = (0u64, 0u64);
        self.plugin.check(unsafe { (f.search_connectivity_f64)(self.ctx, &d, &mut rows, &mut entries) })?;
        let mut off = vec![0u64; rows as usize + 1];
        let mut nb = vec![0u64; entries as usize];
        self.plugin.check(unsafe { (f.search_connectivity_fill)(self.ctx, off.as_mut_ptr(), if entries > 0 { nb.as_mut_ptr() } else { std::ptr::null_mut() }) })?;
        Ok((off.into_iter().map(|v| v as usize).collect(), nb.into_iter().map(|v| v as usize).collect()))
    }

    /// `Modify::unwrap_connectivity_dim` (modify.rs:72-131) with Float = f64, in place: the f64 neighbour search with local ids
    /// under full PBC on the GPU, the reference's stack walk inside the plugin.  Returns the groups of LOCAL indices the
    /// reference returns as selections.
    pub fn unwrap_connectivity_f64(
        &self, coords: &mut [[f64; 3]], index: Option<&[usize]>, box9: &[f64; 9], cutoff: f64, dims: u8,
    ) -> Result<Vec<Vec<usize>>, EngineError> {
        check_index(index, coords.len(), "unwrap_connectivity_f64")?;
        let (ip, n) = idx_ptr(index);
        let nsel = index.map_or(coords.len(), |i| i.len());
        let mut off = vec![0u64; nsel + 1];
        let mut ids = vec![0u64; nsel.max(1)];
        let mut ng = 0usize;
        self.plugin.check(unsafe {
            (self.plugin.fns.unwrap_connectivity_f64)(
                self.ctx, coords.as_mut_ptr() as *mut f64, coords.len(), ip, n, box9.as_ptr(), cutoff, dims, off.as_mut_ptr(),
                ids.as_mut_ptr(), &mut ng,
            )
        })?;
        Ok((0..ng).map(|g| ids[off[g] as usize..off[g + 1] as usize].iter().map(|&v| v as usize).collect()).collect())
    }

    /// `Modify::unwrap_simple_dim` (modify.rs:40-54), in place
    pub fn unwrap_simple_dim(&self, coords: &mut [[f32; 3]], index: Option<&[usize]>, box9: &[f32; 9], dims: u8) -> Result<(), EngineError> {
        check_index(index, coords.len(), "unwrap_simple_dim")?;
        let (ip, n) = idx_ptr(index);
        self.plugin.check(unsafe {
            (self.plugin.fns.unwrap_simple)(self.ctx, coords.as_mut_ptr() as *mut f32, coords.len(), ip, n, box9.as_ptr(), dims)
        })
    }

    /// `Modify::unwrap_connectivity_dim` (modify.rs:72-131), in place: GPU neighbour search with local ids under full PBC,
    /// `SearchConnectivity`'s adjacency in pair order, the reference's stack walk inside the plugin.  Returns the groups of
    /// LOCAL indices the reference returns as selections (`self.select(&sel_vec)`).
    pub fn unwrap_connectivity_dim(
        &self, coords: &mut [[f32; 3]], index: Option<&[usize]>, box9: &[f32; 9], cutoff: f32, dims: u8,
    ) -> Result<Vec<Vec<usize>>, EngineError> {
        check_index(index, coords.len(), "unwrap_connectivity_dim")?;
        let (ip, n) = idx_ptr(index);
        let nsel = index.map_or(coords.len(), |i| i.len());
        let mut off = vec![0u64; nsel + 1];
        let mut ids = vec![0u64; nsel.max(1)];
        let mut ng = 0usize;
        self.plugin.check(unsafe {
            (self.plugin.fns.unwrap_connectivity)(
                self.ctx, coords.as_mut_ptr() as *mut f32, coords.len(), ip, n, box9.as_ptr(), cutoff, dims, off.as_mut_ptr(),
                ids.as_mut_ptr(), &mut ng,
            )
        })?;
        Ok((0..ng).map(|g| ids[off[g] as usize..off[g + 1] as usize].iter().map(|&v| v as usize).collect()).collect())
    }

    /// `Measure::gyration` over a `ParSplit` (system.rs:193-213): selection k is `index[offsets[k]..offsets[k+1]]`.
    pub fn gyration_batch(
        &self, coords: &[[f32; 3]], index: &[usize], offsets: &[usize], masses: &[f32], box9: Option<&[f32; 9]>,
    ) -> Result<Vec<f32>, EngineError> {
        check_index(Some(index), coords.len(), "gyration_batch")?;
        check_offsets(offsets, index.len(), "gyration_batch")?;
        check_column(masses.len(), coords.len(), "gyration_batch: masses")?;
        let nsel = offsets.len().saturating_sub(1);
        let mut out = vec![0f32; nsel];
        self.plugin.check(unsafe {
            (self.plugin.fns.gyration_batch)(self.ctx, coords.as_ptr() as *const f32, coords.len(), index.as_ptr() as *const u64,
                                             offsets.as_ptr() as *const u64, nsel, masses.as_ptr(), box_ptr(box9), out.as_mut_ptr())
        })?;
        Ok(out)
    }

    /// All-pairs minimum RMSD through molar_hip_rmsd_matrix: `rmsd_mw` after the mass-weighted `fit_transform`
    /// (measure.rs:507-522 with :538-558) of every frame of `frames` onto every other one (`frames2` None: the symmetric
    /// matrix, exactly symmetric with a zero diagonal) or onto every frame of `frames2`.  A block holds its frames one after the
    /// other, `natoms` positions each; `masses` None: unit weights; `fit` false: no superposition.  Returns the matrix row by
    /// row, `frames.len() / natoms` rows.
    #[allow(clippy::too_many_arguments)]
    pub fn rmsd_matrix(
        &self, frames: &[[f32; 3]], frames2: Option<&[[f32; 3]]>, natoms: usize, index: Option<&[usize]>, masses: Option<&[f32]>, fit: bool,
    ) -> Result<Vec<f32>, EngineError> {
        check_index(index, natoms, "rmsd_matrix")?;
        if natoms == 0 || frames.len() % natoms != 0 || frames2.is_some_and(|f| f.len() % natoms != 0) {
            return Err(EngineError::Sizes(format!("rmsd_matrix: a block is not a whole number of frames of {natoms} atoms")));
        }
        if let Some(m) = masses {
            check_column(m.len(), natoms, "rmsd_matrix: masses")?;
        }
        let (ip, n) = idx_ptr(index);
        let nsel = if index.is_some() { n } else { natoms };
        if nsel == 0 {
            return Err(EngineError::Sizes("rmsd_matrix: empty selection".into()));
        }
        let f1 = frames.len() / natoms;
        let f2 = frames2.map_or(0, |f| f.len() / natoms);
        let cols = if frames2.is_some() { f2 } else { f1 };
        let mut out = vec![0f32; f1 * cols];
        if out.is_empty() {
            return Ok(out);
        }
        let p2 = frames2.map_or(std::ptr::null(), |f| f.as_ptr() as *const f32);
        let mp = masses.map_or(std::ptr::null(), |m| m.as_ptr());
        self.plugin.check(unsafe {
            (self.plugin.fns.rmsd_matrix)(self.ctx, frames.as_ptr() as *const f32, f1, natoms * 3, p2, f2, natoms * 3, natoms, ip, nsel, mp,
                                          fit as i32, out.as_mut_ptr(), cols)
        })?;
        Ok(out)
    }

    /// Device workspace in bytes and the number of splits of the atom dimension an `rmsd_matrix` call of these sizes uses
    /// (molar_hip_rmsd_matrix_plan, a host function; `nframes2` 0: the symmetric form).
    pub fn rmsd_matrix_plan(&self, nframes1: usize, nframes2: usize, n: usize) -> Result<(usize, u32), EngineError> {
        let (mut ws, mut ks) = (0usize, 0u32);
        self.plugin.check(unsafe { (self.plugin.fns.rmsd_matrix_plan)(nframes1, nframes2, n, &mut ws, &mut ks) })?;
        Ok((ws, ks))
    }

    /// Fluctuations of a block of frames about their mean structure through molar_hip_fluct (the definition: molar_hip.h): the
    /// mean, the per-atom RMSF and, with `want_cov`, the 3n x 3n positional covariance after the mass-weighted fit of every
    /// frame onto `reference` (one position per SELECTED atom; None: frame 0), iterated `iterations` times onto the mean.
    /// `frames` holds whole frames one after the other, `natoms` positions each; `masses` None: unit weights; `fit` false: the
    /// frames as they stand.  With `want_fit` the result also holds, per frame, R (9, column-major), t (3) and the RMSD to
    /// the last reference.
    #[allow(clippy::too_many_arguments)]
    pub fn fluctuations(
        &self, frames: &[[f32; 3]], natoms: usize, index: Option<&[usize]>, masses: Option<&[f32]>, reference: Option<&[[f32; 3]]>, fit: bool,
        iterations: u32, want_cov: bool, want_fit: bool,
    ) -> Result<Fluctuations, EngineError> {
        check_index(index, natoms, "fluctuations")?;
        if natoms == 0 || frames.len() % natoms != 0 {
            return Err(EngineError::Sizes(format!("fluctuations: the block is not a whole number of frames of {natoms} atoms")));
        }
        if let Some(m) = masses {
            check_column(m.len(), natoms, "fluctuations: masses")?;
        }
        let (ip, n) = idx_ptr(index);
        let nsel = if index.is_some() { n } else { natoms };
        if nsel == 0 {
            return Err(EngineError::Sizes("fluctuations: empty selection".into()));
        }
        if let Some(r) = reference {
            if r.len() != nsel {
                return Err(EngineError::Sizes(format!("fluctuations: a reference of {} positions for {nsel} selected atoms", r.len())));
            }
        }
        if iterations > i32::MAX as u32 {
            return Err(EngineError::Sizes("fluctuations: too many iterations".into()));
        }
        let nframes = frames.len() / natoms;
        let mut out = Fluctuations {
            mean: vec![[0f32; 3]; nsel],
            rmsf: vec![0f32; nsel],
            cov: if want_cov { vec![0f32; 9 * nsel * nsel] } else { Vec::new() },
            fit: if want_fit { vec![[0f32; 13]; nframes] } else { Vec::new() },
        };
        if nframes == 0 {
            return Ok(out);
        }
        let mp = masses.map_or(std::ptr::null(), |m| m.as_ptr());
        let rp = reference.map_or(std::ptr::null(), |r| r.as_ptr() as *const f32);
        let cp = if want_cov { out.cov.as_mut_ptr() } else { std::ptr::null_mut() };
        let fp = if want_fit { out.fit.as_mut_ptr() as *mut f32 } else { std::ptr::null_mut() };
        self.plugin.check(unsafe {
            (self.plugin.fns.fluct)(self.ctx, frames.as_ptr() as *const f32, nframes, natoms * 3, natoms, ip, nsel, mp, rp, fit as i32,
                                    iterations as i32, out.mean.as_mut_ptr() as *mut f32, out.rmsf.as_mut_ptr(), cp, 3 * nsel, fp)
        })?;
        Ok(out)
    }

    /// Device workspace in bytes and the number of splits of the frame dimension a `fluctuations` call of these sizes uses
    /// (molar_hip_fluct_plan, a host function).
    pub fn fluct_plan(&self, nframes: usize, n: usize, want_cov: bool) -> Result<(usize, u32), EngineError> {
        let (mut ws, mut ks) = (0usize, 0u32);
        self.plugin.check(unsafe { (self.plugin.fns.fluct_plan)(nframes, n, want_cov as i32, &mut ws, &mut ks) })?;
        Ok((ws, ks))
    }

    /// Mean-squared displacement of a block of frames over all time origins through molar_hip_msd (the definition:
    /// molar_hip.h): every selected atom is followed from frame to frame with the periodic jumps removed (`boxes`: one
    /// column-major box of 9 numbers, or 9 per frame; None: the frames are already unwrapped; `pbc`: the PbcDims byte),
    /// particles are the selected atoms or, with `group_offsets` (CSR over the selection order), the centres of mass of their
    /// groups, and the weighted mean displacement of `ref_index` (the drift) is subtracted when given.  Lags 0 ..= `max_lag`
    /// (None: nframes - 1), origins 0, `origin_stride`, ...; `dims`: the bits x, y, z of the components that enter.
    #[allow(clippy::too_many_arguments)]
    pub fn msd(
        &self, frames: &[[f32; 3]], natoms: usize, index: Option<&[usize]>, masses: Option<&[f32]>, boxes: Option<&[f32]>, pbc: u8,
        group_offsets: Option<&[usize]>, ref_index: Option<&[usize]>, max_lag: Option<usize>, origin_stride: usize, dims: u32, want_particle: bool,
        want_disp: bool,
    ) -> Result<Msd, EngineError> {
        check_index(index, natoms, "msd")?;
        check_index(ref_index, natoms, "msd: reference set")?;
        if natoms == 0 || frames.len() % natoms != 0 {
            return Err(EngineError::Sizes(format!("msd: the block is not a whole number of frames of {natoms} atoms")));
        }
        if let Some(m) = masses {
            check_column(m.len(), natoms, "msd: masses")?;
        }
        let nframes = frames.len() / natoms;
        let (ip, n) = idx_ptr(index);
        let nsel = if index.is_some() { n } else { natoms };
        if nsel == 0 {
            return Err(EngineError::Sizes("msd: empty selection".into()));
        }
        let box_stride = match boxes {
            None => 0,
            Some(b) if b.len() == 9 => 0,
            Some(b) if b.len() == 9 * nframes => 9,
            Some(b) => return Err(EngineError::Sizes(format!("msd: {} box numbers for {nframes} frames", b.len()))),
        };
        let nparticles = match group_offsets {
            Some(g) if g.is_empty() => return Err(EngineError::Sizes("msd: empty group offsets".into())),
            Some(g) => g.len() - 1,
            None => nsel,
        };
        let lags = max_lag.unwrap_or(nframes.saturating_sub(1)) + 1;
        let mut out = Msd {
            msd: vec![0f32; lags],
            m4: vec![0f32; lags],
            msd_particle: if want_particle { vec![0f32; nparticles * lags] } else { Vec::new() },
            disp: if want_disp { vec![[0f32; 3]; nframes * nparticles] } else { Vec::new() },
            nparticles,
        };
        if nframes == 0 {
            return Ok(out);
        }
        let mp = masses.map_or(std::ptr::null(), |m| m.as_ptr());
        let bp = boxes.map_or(std::ptr::null(), |b| b.as_ptr());
        let gp = group_offsets.map_or(std::ptr::null(), |g| g.as_ptr() as *const u64);
        let (rp, nref) = ref_index.map_or((std::ptr::null(), 0), |r| (r.as_ptr() as *const u64, r.len()));
        let pp = if want_particle { out.msd_particle.as_mut_ptr() } else { std::ptr::null_mut() };
        let dp = if want_disp { out.disp.as_mut_ptr() as *mut f32 } else { std::ptr::null_mut() };
        self.plugin.check(unsafe {
            (self.plugin.fns.msd)(self.ctx, frames.as_ptr() as *const f32, nframes, natoms * 3, natoms, ip, nsel, mp, bp, box_stride,
                                  if boxes.is_some() { pbc } else { 0 }, gp, nparticles, rp, nref, lags - 1, origin_stride, dims, out.msd.as_mut_ptr(),
                                  out.m4.as_mut_ptr(), pp, lags, dp)
        })?;
        Ok(out)
    }

    /// Device workspace in bytes, particles per workgroup and lags per workgroup of the lag kernel for an `msd` call of these
    /// sizes (molar_hip_msd_plan, a host function).  `want_lags` false: only the displacements are asked for.
    #[allow(clippy::too_many_arguments)]
    pub fn msd_plan(
        &self, nframes: usize, n: usize, nparticles: usize, nref: usize, max_lag: usize, per_frame_boxes: bool, want_lags: bool,
    ) -> Result<(usize, u32, u32), EngineError> {
        let (mut ws, mut pc, mut lb) = (0usize, 0u32, 0u32);
        self.plugin.check(unsafe {
            (self.plugin.fns.msd_plan)(nframes, n, nparticles, nref, max_lag, per_frame_boxes as i32, want_lags as i32, &mut ws, &mut pc, &mut lb)
        })?;
        Ok((ws, pc, lb))
    }

    /// Density profiles and maps of a block of frames through molar_hip_density (the definition: molar_hip.h): the mean over the
    /// frames of the sum of `weights` (one per ATOM; None: number density) per unit volume in every bin of `grid`, per group
    /// of `labels` ((one label per SELECTED atom, ngroups); None: one group).  `boxes`: one column-major box of 9 numbers, or
    /// 9 per frame (the BOX grids need them); `pbc`: the PbcDims byte; `centre`: (the set a centred grid is centred on in
    /// every frame, its per-ATOM weights or None).  Only integer atomics are used: the same call gives the same bits.
    #[allow(clippy::too_many_arguments)]
    pub fn density(
        &self, frames: &[[f32; 3]], natoms: usize, index: Option<&[usize]>, weights: Option<&[f32]>, labels: Option<(&[u32], usize)>,
        boxes: Option<&[f32]>, pbc: u8, grid: &MolarHipDensityGrid, centre: Option<(&[usize], Option<&[f32]>)>,
    ) -> Result<Density, EngineError> {
        check_index(index, natoms, "density")?;
        check_index(centre.map(|c| c.0), natoms, "density: centre set")?;
        if natoms == 0 || frames.len() % natoms != 0 {
            return Err(EngineError::Sizes(format!("density: the block is not a whole number of frames of {natoms} atoms")));
        }
        if let Some(w) = weights {
            check_column(w.len(), natoms, "density: weights")?;
        }
        if let Some((_, Some(w))) = centre {
            check_column(w.len(), natoms, "density: centre weights")?;
        }
        let nframes = frames.len() / natoms;
        let (ip, n) = idx_ptr(index);
        let nsel = if index.is_some() { n } else { natoms };
        if nsel == 0 {
            return Err(EngineError::Sizes("density: empty selection".into()));
        }
        let box_stride = match boxes {
            None => 0,
            Some(b) if b.len() == 9 => 0,
            Some(b) if b.len() == 9 * nframes => 9,
            Some(b) => return Err(EngineError::Sizes(format!("density: {} box numbers for {nframes} frames", b.len()))),
        };
        let (lp, ngroups) = match labels {
            Some((l, _)) if l.len() != nsel => return Err(EngineError::Sizes(format!("density: {} labels for {nsel} selected atoms", l.len()))),
            Some((l, g)) => (l.as_ptr(), g),
            None => (std::ptr::null(), 1),
        };
        let nb = grid.nbins.iter().map(|&b| b as usize).product::<usize>();
        let mut out = Density {
            density: vec![0f32; ngroups * nb],
            count: vec![0u64; ngroups * nb],
            outside: vec![0u64; nframes],
            centre: vec![[0f32; 3]; nframes],
            binvol: vec![0f32; nframes],
            weight_scale_log2: 0,
            ngroups,
            nbins: nb,
        };
        if nframes == 0 {
            return Ok(out);
        }
        let wp = weights.map_or(std::ptr::null(), |w| w.as_ptr());
        let bp = boxes.map_or(std::ptr::null(), |b| b.as_ptr());
        let (cp, ncentre) = centre.map_or((std::ptr::null(), 0), |c| (c.0.as_ptr() as *const u64, c.0.len()));
        let cwp = centre.and_then(|c| c.1).map_or(std::ptr::null(), |w| w.as_ptr());
        self.plugin.check(unsafe {
            (self.plugin.fns.density)(self.ctx, frames.as_ptr() as *const f32, nframes, natoms * 3, natoms, ip, nsel, wp, lp, ngroups, bp, box_stride, pbc,
                                      grid as *const MolarHipDensityGrid, cp, ncentre, cwp, out.density.as_mut_ptr(), out.count.as_mut_ptr(),
                                      out.outside.as_mut_ptr(), out.centre.as_mut_ptr() as *mut f32, out.binvol.as_mut_ptr(), &mut out.weight_scale_log2)
        })?;
        Ok(out)
    }

    /// Device workspace in bytes, the frames whose integer bins are held at once, the atoms of one frame per workgroup of the
    /// binning kernels and the largest ngroups * bins the on-chip kernel takes, for a `density` call of these sizes
    /// (molar_hip_density_plan, a host function).
    pub fn density_plan(&self, nframes: usize, n: usize, ngroups: usize, grid: &MolarHipDensityGrid) -> Result<(usize, u32, u32, u32), EngineError> {
        let (mut ws, mut fc, mut ac, mut lc) = (0usize, 0u32, 0u32, 0u32);
        self.plugin.check(unsafe {
            (self.plugin.fns.density_plan)(nframes, n, ngroups, grid as *const MolarHipDensityGrid, &mut ws, &mut fc, &mut ac, &mut lc)
        })?;
        Ok((ws, fc, ac, lc))
    }

    /// Distances, angles or dihedrals (radians) of `tuples` (`spec.kind` atom indices each) in every frame of a block through
    /// molar_hip_intcoord (the definition: molar_hip.h): the series, the histograms per group of `labels` ((one label per tuple,
    /// ngroups); None: one group), the joint histogram of the two tuples of every pair of `pairs` ((pairs, their labels and
    /// groups or None): the Ramachandran map), and the mean, the spread (dihedrals: the circular variance) and the valid frames
    /// per tuple.  `boxes`: one column-major box of 9 numbers or 9 per frame, every bond vector then takes its minimum image on
    /// the dimensions of `pbc`; None: no image is removed.  Only integer atomics are used: the same call gives the same bits.
    #[allow(clippy::too_many_arguments)]
    pub fn internal_coords(
        &self, frames: &[[f32; 3]], natoms: usize, tuples: &[usize], labels: Option<(&[u32], usize)>, boxes: Option<&[f32]>, pbc: u8,
        spec: &MolarHipIntcoordSpec, pairs: Option<(&[[usize; 2]], Option<(&[u32], usize)>)>,
    ) -> Result<InternalCoords, EngineError> {
        let kind = spec.kind as usize;
        if !(2..=4).contains(&kind) || tuples.len() % kind != 0 {
            return Err(EngineError::Sizes(format!("internal_coords: {} indices are not tuples of {kind} atoms", tuples.len())));
        }
        if natoms == 0 || frames.len() % natoms != 0 {
            return Err(EngineError::Sizes(format!("internal_coords: the block is not a whole number of frames of {natoms} atoms")));
        }
        check_index(Some(tuples), natoms, "internal_coords")?;
        let nframes = frames.len() / natoms;
        let ntuples = tuples.len() / kind;
        let box_stride = match boxes {
            None => 0,
            Some(b) if b.len() == 9 => 0,
            Some(b) if b.len() == 9 * nframes => 9,
            Some(b) => return Err(EngineError::Sizes(format!("internal_coords: {} box numbers for {nframes} frames", b.len()))),
        };
        let (lp, ngroups) = match labels {
            Some((l, _)) if l.len() != ntuples => return Err(EngineError::Sizes(format!("internal_coords: {} labels for {ntuples} tuples", l.len()))),
            Some((l, g)) => (l.as_ptr(), g),
            None => (std::ptr::null(), 1),
        };
        let want_map = spec.map_bins != 0 && pairs.is_some();
        let (pp, npairs, plp, npair_groups) = match pairs {
            Some((p, Some((l, _)))) if l.len() != p.len() => return Err(EngineError::Sizes(format!("internal_coords: {} labels for {} pairs", l.len(), p.len()))),
            Some((p, Some((l, g)))) if want_map => (p.as_ptr() as *const u64, p.len(), l.as_ptr(), g),
            Some((p, None)) if want_map => (p.as_ptr() as *const u64, p.len(), std::ptr::null(), 1),
            _ => (std::ptr::null(), 0, std::ptr::null(), 1),
        };
        let (nbins, mb) = (spec.nbins as usize, spec.map_bins as usize);
        let mut out = InternalCoords {
            values: vec![0f32; nframes * ntuples],
            hist: vec![0u64; ngroups * nbins],
            map: vec![0u64; if want_map { npair_groups * mb * mb } else { 0 }],
            mean: vec![0f32; ntuples],
            spread: vec![0f32; ntuples],
            valid: vec![0u64; ntuples],
            nframes,
            ntuples,
            ngroups,
            npair_groups,
        };
        if nframes == 0 || ntuples == 0 {
            return Ok(out);
        }
        let bp = boxes.map_or(std::ptr::null(), |b| b.as_ptr());
        let hp = if nbins != 0 { out.hist.as_mut_ptr() } else { std::ptr::null_mut() };
        let mp = if want_map { out.map.as_mut_ptr() } else { std::ptr::null_mut() };
        self.plugin.check(unsafe {
            (self.plugin.fns.intcoord)(self.ctx, frames.as_ptr() as *const f32, nframes, natoms * 3, natoms, tuples.as_ptr() as *const u64, ntuples, lp, ngroups, bp,
                                       box_stride, if boxes.is_some() { pbc } else { 0 }, spec as *const MolarHipIntcoordSpec, pp, npairs, plp, npair_groups,
                                       out.values.as_mut_ptr(), ntuples, hp, mp, out.mean.as_mut_ptr(), out.spread.as_mut_ptr(), out.valid.as_mut_ptr())
        })?;
        Ok(out)
    }

    /// Device workspace in bytes, the frames and the tuples (or pairs) a workgroup takes and the largest groups * bins the
    /// on-chip histogram takes, for an `internal_coords` call of these sizes (molar_hip_intcoord_plan, a host function).
    #[allow(clippy::too_many_arguments)]
    pub fn internal_coords_plan(
        &self, nframes: usize, ntuples: usize, ngroups: usize, npairs: usize, npair_groups: usize, spec: &MolarHipIntcoordSpec, want_stats: bool,
    ) -> Result<(usize, u32, u32, u32), EngineError> {
        let (mut ws, mut fc, mut tc, mut lc) = (0usize, 0u32, 0u32, 0u32);
        self.plugin.check(unsafe {
            (self.plugin.fns.intcoord_plan)(nframes, ntuples, ngroups, npairs, npair_groups, spec as *const MolarHipIntcoordSpec, want_stats as i32, &mut ws, &mut fc,
                                            &mut tc, &mut lc)
        })?;
        Ok((ws, fc, tc, lc))
    }

    /// Time correlation functions of the vectors of `tuples` (`spec.kind` atom indices each: 1 the atom's own 3-vector, 2 the
    /// bond vector, 3 the plane normal) over all time origins of a block of frames through molar_hip_tcf (the definition:
    /// molar_hip.h): c1 and c2 (the first and second Legendre polynomial of u(t) . u(t + tau)) per group of `labels` ((one label
    /// per vector, ngroups); None: one group) for the lags 0 ..= `max_lag` and the origins 0, `origin_stride`, ..., per vector
    /// as well with `per_vector`, and the mean vector, the order parameter S^2 and the bad frames of every vector.  `boxes`:
    /// one column-major box of 9 numbers or 9 per frame, every bond vector then takes its minimum image on the dimensions of
    /// `pbc`; None: no image is removed.  In RAW mode c2, c2_vec and s2 stay empty.  No floating-point atomics are used: the
    /// same call gives the same bits.
    #[allow(clippy::too_many_arguments)]
    pub fn vector_correlations(
        &self, frames: &[[f32; 3]], natoms: usize, tuples: &[usize], labels: Option<(&[u32], usize)>, boxes: Option<&[f32]>, pbc: u8,
        spec: &MolarHipTcfSpec, max_lag: usize, origin_stride: usize, per_vector: bool,
    ) -> Result<VectorCorrelations, EngineError> {
        let kind = spec.kind as usize;
        if !(1..=3).contains(&kind) || tuples.len() % kind != 0 {
            return Err(EngineError::Sizes(format!("vector_correlations: {} indices are not tuples of {kind} atoms", tuples.len())));
        }
        if natoms == 0 || frames.len() % natoms != 0 {
            return Err(EngineError::Sizes(format!("vector_correlations: the block is not a whole number of frames of {natoms} atoms")));
        }
        check_index(Some(tuples), natoms, "vector_correlations")?;
        let nframes = frames.len() / natoms;
        let nvectors = tuples.len() / kind;
        let use_box = boxes.is_some() && kind >= 2;
        let box_stride = match boxes {
            None => 0,
            Some(b) if b.len() == 9 => 0,
            Some(b) if b.len() == 9 * nframes => 9,
            Some(b) => return Err(EngineError::Sizes(format!("vector_correlations: {} box numbers for {nframes} frames", b.len()))),
        };
        let (lp, ngroups) = match labels {
            Some((l, _)) if l.len() != nvectors => return Err(EngineError::Sizes(format!("vector_correlations: {} labels for {nvectors} vectors", l.len()))),
            Some((l, g)) => (l.as_ptr(), g),
            None => (std::ptr::null(), 1),
        };
        let unit = spec.mode == TCF_UNIT;
        let nlags = max_lag + 1;
        let mut out = VectorCorrelations {
            c1: vec![0f32; ngroups * nlags],
            c2: vec![0f32; if unit { ngroups * nlags } else { 0 }],
            c1_vec: vec![0f32; if per_vector { nvectors * nlags } else { 0 }],
            c2_vec: vec![0f32; if per_vector && unit { nvectors * nlags } else { 0 }],
            nvalid: vec![0u64; ngroups],
            mean: vec![0f32; nvectors * 3],
            s2: vec![0f32; if unit { nvectors } else { 0 }],
            bad_frames: vec![0u32; nvectors],
            nframes,
            nvectors,
            ngroups,
            nlags,
        };
        if nframes == 0 {
            return Ok(out);
        }
        fn ptr<T>(v: &mut Vec<T>) -> *mut T {
            if v.is_empty() { std::ptr::null_mut() } else { v.as_mut_ptr() }
        }
        let bp = if use_box { boxes.map_or(std::ptr::null(), |b| b.as_ptr()) } else { std::ptr::null() };
        self.plugin.check(unsafe {
            (self.plugin.fns.tcf)(self.ctx, frames.as_ptr() as *const f32, nframes, natoms * 3, natoms, tuples.as_ptr() as *const u64, nvectors, lp, ngroups, bp,
                                  box_stride, if use_box { pbc } else { 0 }, spec as *const MolarHipTcfSpec, max_lag, origin_stride, ptr(&mut out.c1),
                                  ptr(&mut out.c2), ptr(&mut out.c1_vec), ptr(&mut out.c2_vec), nlags, ptr(&mut out.nvalid), ptr(&mut out.mean),
                                  ptr(&mut out.s2), ptr(&mut out.bad_frames))
        })?;
        Ok(out)
    }

    /// Device workspace in bytes and the launch shape (frame_chunk, vec_chunk, lag_block, lags_per_lane, segment, window) of a
    /// `vector_correlations` call of these sizes (molar_hip_tcf_plan, a host function).
    #[allow(clippy::too_many_arguments)]
    pub fn vector_correlations_plan(
        &self, nframes: usize, nvectors: usize, ngroups: usize, max_lag: usize, per_frame_boxes: bool, want_lags: bool, want_groups: bool,
    ) -> Result<(usize, [u32; 6]), EngineError> {
        let mut ws = 0usize;
        let mut s = [0u32; 6];
        let p = s.as_mut_ptr();
        self.plugin.check(unsafe {
            (self.plugin.fns.tcf_plan)(nframes, nvectors, ngroups, max_lag, per_frame_boxes as i32, want_lags as i32, want_groups as i32, &mut ws, p, p.add(1),
                                       p.add(2), p.add(3), p.add(4), p.add(5))
        })?;
        Ok((ws, s))
    }

    /// Static structure factors of a block of frames through molar_hip_sfactor (the definition: molar_hip.h): the collective
    /// density rho_g(m) of every group of `labels` ((one label per selected atom, ngroups); None: one group) over the reciprocal
    /// lattice of `boxes` (one column-major matrix of 9 numbers or 9 per frame) up to the Miller indices of `grid`, h >= 0 only,
    /// with `weight` (one per ATOM, of any sign; None: 1) - per frame with `want_rho`, its mean over the ok frames with
    /// `want_mean` - the partial products S_ab for a <= b, not normalised, and their average over the shells of |q| of `grid`.
    /// A frame with a selected coordinate that is not finite is 0 in `frame_ok`, NaN in rho and enters no average.  No
    /// floating-point atomics are used: the same call gives the same bits.
    #[allow(clippy::too_many_arguments)]
    pub fn structure_factor(
        &self, frames: &[[f32; 3]], natoms: usize, idx: Option<&[usize]>, weight: Option<&[f32]>, labels: Option<(&[u32], usize)>, boxes: &[f32],
        grid: &MolarHipSfactorGrid, want_rho: bool, want_mean: bool,
    ) -> Result<StructureFactor, EngineError> {
        if natoms == 0 || frames.len() % natoms != 0 {
            return Err(EngineError::Sizes(format!("structure_factor: the block is not a whole number of frames of {natoms} atoms")));
        }
        check_index(idx, natoms, "structure_factor")?;
        let nframes = frames.len() / natoms;
        let n = idx.map_or(natoms, |i| i.len());
        let box_stride = match boxes.len() {
            9 => 0,
            l if l == 9 * nframes => 9,
            l => return Err(EngineError::Sizes(format!("structure_factor: {l} box numbers for {nframes} frames"))),
        };
        if let Some(w) = weight {
            if w.len() != natoms {
                return Err(EngineError::Sizes(format!("structure_factor: {} weights for {natoms} atoms", w.len())));
            }
        }
        let (lp, ngroups) = match labels {
            Some((l, _)) if l.len() != n => return Err(EngineError::Sizes(format!("structure_factor: {} labels for {n} selected atoms", l.len()))),
            Some((l, g)) => (l.as_ptr(), g),
            None => (std::ptr::null(), 1),
        };
        let nq = (grid.hmax[0] as usize + 1) * (2 * grid.hmax[1] as usize + 1) * (2 * grid.hmax[2] as usize + 1);
        let npairs = ngroups * (ngroups + 1) / 2;
        let nshells = grid.nshells as usize;
        let mut out = StructureFactor {
            rho: vec![0f32; if want_rho { nframes * ngroups * nq * 2 } else { 0 }],
            frame_ok: vec![0u32; nframes],
            rho_mean: vec![0f32; if want_mean { ngroups * nq * 2 } else { 0 }],
            sab: vec![0f32; npairs * nq],
            shell: vec![0f32; npairs * nshells],
            shell_count: vec![0u64; nshells],
            nframes,
            ngroups,
            npairs,
            nq,
            nshells,
        };
        if nframes == 0 {
            return Ok(out);
        }
        fn ptr<T>(v: &mut Vec<T>) -> *mut T {
            if v.is_empty() { std::ptr::null_mut() } else { v.as_mut_ptr() }
        }
        self.plugin.check(unsafe {
            (self.plugin.fns.sfactor)(self.ctx, frames.as_ptr() as *const f32, nframes, natoms * 3, natoms, idx.map_or(std::ptr::null(), |i| i.as_ptr() as *const u64),
                                      n, weight.map_or(std::ptr::null(), |w| w.as_ptr()), lp, ngroups, boxes.as_ptr(), box_stride,
                                      grid as *const MolarHipSfactorGrid, ptr(&mut out.rho), 2 * nq, ptr(&mut out.frame_ok), ptr(&mut out.rho_mean),
                                      ptr(&mut out.sab), ptr(&mut out.shell), ptr(&mut out.shell_count))
        })?;
        Ok(out)
    }

    /// Device workspace in bytes and the launch shape (layout, row_block, col_block, atom_chunk, ksplits, frame_block) of a
    /// `structure_factor` call of these sizes (molar_hip_sfactor_plan, a host function).
    pub fn structure_factor_plan(&self, nframes: usize, n: usize, ngroups: usize, grid: &MolarHipSfactorGrid) -> Result<(usize, [u32; 6]), EngineError> {
        let mut ws = 0usize;
        let mut s = [0u32; 6];
        let p = s.as_mut_ptr();
        self.plugin.check(unsafe {
            (self.plugin.fns.sfactor_plan)(nframes, n, ngroups, grid as *const MolarHipSfactorGrid, &mut ws, p, p.add(1), p.add(2), p.add(3), p.add(4), p.add(5))
        })?;
        Ok((ws, s))
    }

    /// Minimum distances between two selections of a block of frames through molar_hip_mindist (the definition: molar_hip.h):
    /// every pair under the minimum image of `boxes` (None: plain differences; one column-major matrix of 9 numbers or 9 per
    /// frame) with the mask `spec.pbc`.  `idx1` / `idx2`: the sets (None: atoms 0 .. natoms - 1); `spec.same` = 1: set 2 is set
    /// 1 (`idx2`, `labels2` stay None).  `labels1` / `labels2`: (one label per selected atom, ngroups), None: one group.  `want`:
    /// the sum of MINDIST_DIST (dist, pair), MINDIST_ATOM1 (atom1, near1), MINDIST_ATOM2 and MINDIST_MAT (mat, mat_mean, mat_min,
    /// mat_freq).  Positions are those within the sets; without a pair a distance is +inf and a position u64::MAX; a frame
    /// with a selected coordinate that is not finite, or a refused box, is 0 in `frame_ok`, NaN in every per-frame result and
    /// enters no reduction.  Only minima under a total order and sums in frame order: the same call gives the same bits.
    #[allow(clippy::too_many_arguments)]
    pub fn min_distances(
        &self, frames: &[[f32; 3]], natoms: usize, idx1: Option<&[usize]>, idx2: Option<&[usize]>, labels1: Option<(&[u32], usize)>,
        labels2: Option<(&[u32], usize)>, boxes: Option<&[f32]>, spec: &MolarHipMindistSpec, want: u32,
    ) -> Result<MinDistances, EngineError> {
        if natoms == 0 || frames.len() % natoms != 0 {
            return Err(EngineError::Sizes(format!("min_distances: the block is not a whole number of frames of {natoms} atoms")));
        }
        check_index(idx1, natoms, "min_distances")?;
        check_index(idx2, natoms, "min_distances")?;
        let nframes = frames.len() / natoms;
        let n1 = idx1.map_or(natoms, |i| i.len());
        let n2 = if spec.same != 0 { n1 } else { idx2.map_or(natoms, |i| i.len()) };
        let box_stride = match boxes.map_or(9, |b| b.len()) {
            9 => 0,
            l if l == 9 * nframes => 9,
            l => return Err(EngineError::Sizes(format!("min_distances: {l} box numbers for {nframes} frames"))),
        };
        let (l1, g1) = match labels1 {
            Some((l, _)) if l.len() != n1 => return Err(EngineError::Sizes(format!("min_distances: {} labels for {n1} atoms of set 1", l.len()))),
            Some((l, g)) => (l.as_ptr(), g),
            None => (std::ptr::null(), 1),
        };
        let (l2, g2) = match labels2 {
            Some((l, _)) if l.len() != n2 => return Err(EngineError::Sizes(format!("min_distances: {} labels for {n2} atoms of set 2", l.len()))),
            Some((l, g)) => (l.as_ptr(), g),
            None => (std::ptr::null(), if spec.same != 0 { g1 } else { 1 }),
        };
        let cells = g1 * g2;
        let on = |bit: u32, len: usize| if want & bit != 0 { len } else { 0 };
        let mut out = MinDistances {
            dist: vec![0f32; on(MINDIST_DIST, nframes)],
            pair: vec![0u64; on(MINDIST_DIST, 2 * nframes)],
            atom1: vec![0f32; on(MINDIST_ATOM1, nframes * n1)],
            near1: vec![0u64; on(MINDIST_ATOM1, nframes * n1)],
            atom2: vec![0f32; on(MINDIST_ATOM2, nframes * n2)],
            mat: vec![0f32; on(MINDIST_MAT, nframes * cells)],
            mat_mean: vec![0f64; on(MINDIST_MAT, cells)],
            mat_min: vec![0f32; on(MINDIST_MAT, cells)],
            mat_freq: vec![0u32; on(MINDIST_MAT, cells)],
            frame_ok: vec![0u32; nframes],
            nvalid: 0,
            nframes,
            n1,
            n2,
            ngroups1: g1,
            ngroups2: g2,
        };
        if nframes == 0 {
            return Ok(out);
        }
        fn ptr<T>(v: &mut Vec<T>) -> *mut T {
            if v.is_empty() { std::ptr::null_mut() } else { v.as_mut_ptr() }
        }
        let mut sp = *spec;
        if boxes.is_none() {
            sp.pbc = 0;
        }
        self.plugin.check(unsafe {
            (self.plugin.fns.mindist)(self.ctx, frames.as_ptr() as *const f32, nframes, natoms * 3, natoms, idx1.map_or(std::ptr::null(), |i| i.as_ptr() as *const u64),
                                      n1, l1, g1, idx2.map_or(std::ptr::null(), |i| i.as_ptr() as *const u64), n2, l2, g2,
                                      boxes.map_or(std::ptr::null(), |b| b.as_ptr()), box_stride, &sp as *const MolarHipMindistSpec, ptr(&mut out.dist),
                                      ptr(&mut out.pair), ptr(&mut out.atom1), ptr(&mut out.near1), n1, ptr(&mut out.atom2), n2, ptr(&mut out.mat),
                                      ptr(&mut out.mat_mean), ptr(&mut out.mat_min), ptr(&mut out.mat_freq), ptr(&mut out.frame_ok), &mut out.nvalid)
        })?;
        Ok(out)
    }

    /// Device workspace in bytes and the launch shape (rows_per_wave, rows_per_block, cols_per_tile, col_splits, frame_block) of a
    /// `min_distances` call of these sizes asked for `want` (molar_hip_mindist_plan, a host function).
    pub fn min_distances_plan(&self, nframes: usize, n1: usize, n2: usize, ngroups1: usize, ngroups2: usize, spec: &MolarHipMindistSpec, want: u32)
        -> Result<(usize, [u32; 5]), EngineError> {
        let mut ws = 0usize;
        let mut s = [0u32; 5];
        let p = s.as_mut_ptr();
        self.plugin.check(unsafe {
            (self.plugin.fns.mindist_plan)(nframes, n1, n2, ngroups1, ngroups2, spec as *const MolarHipMindistSpec, want, &mut ws, p, p.add(1), p.add(2), p.add(3),
                                           p.add(4))
        })?;
        Ok((ws, s))
    }

    /// The self part of the van Hove function through molar_hip_vanhove (the definition: molar_hip.h) of an ALREADY UNWRAPPED
    /// particle trajectory `traj` (frames of `natoms` particles: the `disp` of `msd`, or raw coordinates of a system that is not
    /// periodic; no box is taken): the displacements over `lags` (strictly increasing, below the number of frames, 0 allowed) and
    /// the origins 0, `spec.origin_stride`, ..., counted into `spec.nbins` bins of [`spec.lo`, `spec.hi`) per group.  `idx`:
    /// the selection (None: every particle); `labels`: (one label per selected particle, ngroups), None: one group.  A particle
    /// with a coordinate of `spec.dims` that is not finite enters no count.  Every result is an integer: the same call gives
    /// the same bits.
    pub fn van_hove(
        &self, traj: &[[f32; 3]], natoms: usize, idx: Option<&[usize]>, labels: Option<(&[u32], usize)>, lags: &[u64], spec: &VanHoveSpec,
    ) -> Result<VanHove, EngineError> {
        if natoms == 0 || traj.len() % natoms != 0 {
            return Err(EngineError::Sizes(format!("van_hove: the block is not a whole number of frames of {natoms} particles")));
        }
        check_index(idx, natoms, "van_hove")?;
        let nframes = traj.len() / natoms;
        let n = idx.map_or(natoms, |i| i.len());
        let (lp, g) = match labels {
            Some((l, _)) if l.len() != n => return Err(EngineError::Sizes(format!("van_hove: {} labels for {n} particles", l.len()))),
            Some((l, g)) => (l.as_ptr(), g),
            None => (std::ptr::null(), 1),
        };
        if lags.is_empty() || n == 0 || g == 0 {
            return Err(EngineError::Sizes("van_hove: no lags, no particles or no groups".into()));
        }
        if lags.windows(2).any(|w| w[1] <= w[0]) || (nframes > 0 && lags[lags.len() - 1] >= nframes as u64) {
            return Err(EngineError::Sizes(format!("van_hove: the lags must increase strictly and stay below the {nframes} frames")));
        }
        let ndims = (spec.dims & 7).count_ones();
        if spec.dims == 0 || spec.dims > 7 || spec.flags & !VANHOVE_SIGNED != 0 || (spec.flags & VANHOVE_SIGNED != 0 && ndims != 1) {
            return Err(EngineError::Sizes(format!("van_hove: dims = {} with flags = {}", spec.dims, spec.flags)));
        }
        if !(spec.lo.is_finite() && spec.hi.is_finite() && spec.lo < spec.hi) || spec.nbins == 0 || spec.origin_stride == 0 {
            return Err(EngineError::Sizes("van_hove: a finite range lo < hi, nbins >= 1 and origin_stride >= 1 are needed".into()));
        }
        let cells = g.checked_mul(lags.len()).and_then(|c| c.checked_mul(spec.nbins)).filter(|&c| c < 1usize << 31);
        let cells = cells.ok_or_else(|| EngineError::Sizes("van_hove: 2^31 histogram cells or more".into()))?;
        let mut out = VanHove {
            hist: vec![0u64; cells],
            outside: vec![0u64; g * lags.len()],
            norigins: vec![0u64; lags.len()],
            nvalid: vec![0u64; g],
            bad: vec![0u32; n],
            edges: (0..=spec.nbins).map(|b| spec.lo + (spec.hi - spec.lo) * b as f64 / spec.nbins as f64).collect(),
            ngroups: g,
            nlags: lags.len(),
            nbins: spec.nbins,
        };
        if nframes == 0 {
            return Ok(out);
        }
        self.plugin.check(unsafe {
            (self.plugin.fns.vanhove)(self.ctx, traj.as_ptr() as *const f32, nframes, natoms * 3, natoms, idx.map_or(std::ptr::null(), |i| i.as_ptr() as *const u64), n,
                                      lp, g, lags.as_ptr(), lags.len(), spec.origin_stride, spec.dims, spec.flags, spec.lo, spec.hi, spec.nbins,
                                      out.hist.as_mut_ptr(), out.outside.as_mut_ptr(), out.norigins.as_mut_ptr(), out.nvalid.as_mut_ptr(), out.bad.as_mut_ptr())
        })?;
        Ok(out)
    }

    /// The device workspace and the launch shape of a `van_hove` call of these sizes (molar_hip_vanhove_plan, a host function);
    /// `ndims`: the components that enter (1, 2 or 3).
    pub fn van_hove_plan(&self, nframes: usize, n: usize, ngroups: usize, nlags: usize, nbins: usize, ndims: u32) -> Result<VanHovePlan, EngineError> {
        let mut p = VanHovePlan::default();
        self.plugin.check(unsafe {
            (self.plugin.fns.vanhove_plan)(nframes, n, ngroups, nlags, nbins, ndims, &mut p.workspace_bytes, &mut p.particles_per_wg, &mut p.origins_per_pass,
                                           &mut p.lag_tile, &mut p.on_chip, &mut p.lds_cells, &mut p.pass_splits, &mut p.pairs_per_flush)
        })?;
        Ok(p)
    }

    /// Lifetime correlations of a sparse presence matrix frames x rows (`molar_hip_lifetimes`; the definition is in the header):
    /// the rows present in frame t are `row_of_entry[frame_offsets[t] .. frame_offsets[t + 1]]`.  `labels`: (one label per row,
    /// ngroups), None: one group.  Lags 0 ..= `max_lag`, origins 0, `origin_stride`, ...; `gap`: zero runs of at most that many
    /// frames between two present frames are filled first.
    #[allow(clippy::too_many_arguments)]
    pub fn lifetimes(
        &self, frame_offsets: &[u64], row_of_entry: &[u32], nrows: usize, labels: Option<(&[u32], usize)>, max_lag: usize,
        origin_stride: usize, gap: usize,
    ) -> Result<Lifetimes, EngineError> {
        if frame_offsets.is_empty() {
            return Err(EngineError::Sizes("lifetimes: frame_offsets is empty".into()));
        }
        let nframes = frame_offsets.len() - 1;
        if frame_offsets[nframes] as usize != row_of_entry.len() {
            return Err(EngineError::Sizes("lifetimes: frame_offsets must end at row_of_entry.len()".into()));
        }
        let (gp, ngroups) = lifetime_labels("lifetimes", labels, nrows)?;
        let mut out = Lifetimes::sized(nframes, nrows, ngroups, max_lag, origin_stride);
        let rp = if row_of_entry.is_empty() { std::ptr::null() } else { row_of_entry.as_ptr() };
        self.plugin.check(unsafe {
            (self.plugin.fns.lifetimes)(self.ctx, frame_offsets.as_ptr(), rp, nframes, nrows, gp, ngroups, max_lag, origin_stride, gap,
                                        out.inter.as_mut_ptr(), out.cont.as_mut_ptr(), out.run_hist.as_mut_ptr(), out.events.as_mut_ptr(),
                                        out.longest.as_mut_ptr(), out.present.as_mut_ptr())
        })?;
        Ok(out)
    }

    /// (frames, rows of the bond table, entries, serial number) of the block this engine keeps after `molar_hip_hbonds_frames`
    /// (`molar_hip_hbonds_frames_shape`); an error without one.
    pub fn hbonds_frames_shape(&self) -> Result<(usize, usize, usize, u64), EngineError> {
        let (mut nframes, mut nrows, mut nentries, mut serial) = (0usize, 0usize, 0usize, 0u64);
        self.plugin.check(unsafe { (self.plugin.fns.hbonds_frames_shape)(self.ctx, &mut nframes, &mut nrows, &mut nentries, &mut serial) })?;
        Ok((nframes, nrows, nentries, serial))
    }

    /// The same on the block this engine keeps after `molar_hip_hbonds_frames` (`molar_hip_hbonds_frames_lifetimes`), read where it
    /// lies on the device.  The outputs are sized by the frames and rows the LIBRARY reports for that block (`hbonds_frames_shape`,
    /// in the same borrow of the engine), never by numbers of the caller's; `labels` must have one entry per row of that block.
    pub fn hbonds_frames_lifetimes(
        &self, labels: Option<(&[u32], usize)>, max_lag: usize, origin_stride: usize, gap: usize,
    ) -> Result<Lifetimes, EngineError> {
        let (nframes, nrows, _, _) = self.hbonds_frames_shape()?;
        let (gp, ngroups) = lifetime_labels("hbonds_frames_lifetimes", labels, nrows)?;
        let mut out = Lifetimes::sized(nframes, nrows, ngroups, max_lag, origin_stride);
        self.plugin.check(unsafe {
            (self.plugin.fns.hbonds_frames_lifetimes)(self.ctx, gp, ngroups, max_lag, origin_stride, gap, out.inter.as_mut_ptr(),
                                                      out.cont.as_mut_ptr(), out.run_hist.as_mut_ptr(), out.events.as_mut_ptr(),
                                                      out.longest.as_mut_ptr(), out.present.as_mut_ptr())
        })?;
        Ok(out)
    }

    /// Device workspace in bytes and 64-bit words per row of a `lifetimes` call of these sizes (molar_hip_lifetimes_plan, a host
    /// function).
    pub fn lifetimes_plan(&self, nframes: usize, nrows: usize, ngroups: usize, want_cont: bool) -> Result<(usize, u32), EngineError> {
        let (mut ws, mut wpr) = (0usize, 0u32);
        self.plugin.check(unsafe { (self.plugin.fns.lifetimes_plan)(nframes, nrows, ngroups, want_cont as i32, &mut ws, &mut wpr) })?;
        Ok((ws, wpr))
    }
}

fn lifetime_labels(who: &str, labels: Option<(&[u32], usize)>, nrows: usize) -> Result<(*const u32, usize), EngineError> {
    match labels {
        None => Ok((std::ptr::null(), 1)),
        Some((g, _)) if g.len() != nrows => Err(EngineError::Sizes(format!("{who}: one label per row"))),
        Some((g, ngroups)) => Ok((g.as_ptr(), ngroups)),
    }
}

/// What `Engine::lifetimes` returns: the numerators of the intermittent and the continuous correlation [ngroups][max_lag + 1],
/// the runs by length [ngroups][nframes + 1], per row the runs, the longest run and the present frames, and `count[tau]`, the
/// time origins of every lag: C(tau) = (x[tau] / count[tau]) / (x[0] / count[0]).
#[derive(Debug, Clone, Default)]
pub struct Lifetimes {
    pub inter: Vec<u64>,
    pub cont: Vec<u64>,
    pub run_hist: Vec<u64>,
    pub events: Vec<u32>,
    pub longest: Vec<u32>,
    pub present: Vec<u32>,
    pub count: Vec<u64>,
    pub ngroups: usize,
}

impl Lifetimes {
    fn sized(nframes: usize, nrows: usize, ngroups: usize, max_lag: usize, origin_stride: usize) -> Self {
        let lags = max_lag + 1;
        let count = if origin_stride > 0 && max_lag < nframes {
            (0..lags).map(|tau| ((nframes - 1 - tau) / origin_stride + 1) as u64).collect()
        } else {
            Vec::new()
        };
        Lifetimes {
            inter: vec![0; ngroups * lags], cont: vec![0; ngroups * lags], run_hist: vec![0; ngroups * (nframes + 1)],
            events: vec![0; nrows], longest: vec![0; nrows], present: vec![0; nrows], count, ngroups,
        }
    }
}

/// What `Engine::msd` returns: MSD and fourth moment per lag, the per-particle curves row by row and the unwrapped particle
/// displacements [frame][particle] relative to frame 0 (the last two empty unless asked for).
#[derive(Debug, Clone, Default)]
pub struct Msd {
    pub msd: Vec<f32>,
    pub m4: Vec<f32>,
    pub msd_particle: Vec<f32>,
    pub disp: Vec<[f32; 3]>,
    pub nparticles: usize,
}

/// What `Engine::density` returns: the density [group][bin] (bin (bx ny + by) nz + bz), the atoms counted per group and bin over
/// the block, per frame the selected atoms that were dropped, the centre used and the bin volume, and the scale of the weights.
#[derive(Debug, Clone, Default)]
pub struct Density {
    pub density: Vec<f32>,
    pub count: Vec<u64>,
    pub outside: Vec<u64>,
    pub centre: Vec<[f32; 3]>,
    pub binvol: Vec<f32>,
    pub weight_scale_log2: i32,
    pub ngroups: usize,
    pub nbins: usize,
}

/// What `Engine::internal_coords` returns: the series [frame][tuple] (NaN where invalid), the histogram [group][bin] (empty
/// without bins), the map [pair group][bin of the first][bin of the second] (empty without map bins or pairs), and per tuple the
/// mean, the spread and the frames that entered.
#[derive(Debug, Clone, Default)]
pub struct InternalCoords {
    pub values: Vec<f32>,
    pub hist: Vec<u64>,
    pub map: Vec<u64>,
    pub mean: Vec<f32>,
    pub spread: Vec<f32>,
    pub valid: Vec<u64>,
    pub nframes: usize,
    pub ntuples: usize,
    pub ngroups: usize,
    pub npair_groups: usize,
}

/// What `Engine::vector_correlations` returns: c1 and c2 [group][lag] (a group without a valid vector: NaN), c1_vec and c2_vec
/// [vector][lag] (empty unless asked for), the valid vectors per group, and per vector the mean [3], the order parameter S^2 and
/// the bad frames; c2, c2_vec and s2 are empty in RAW mode.  A vector with a bad frame is NaN in its own rows.
#[derive(Debug, Clone, Default)]
pub struct VectorCorrelations {
    pub c1: Vec<f32>,
    pub c2: Vec<f32>,
    pub c1_vec: Vec<f32>,
    pub c2_vec: Vec<f32>,
    pub nvalid: Vec<u64>,
    pub mean: Vec<f32>,
    pub s2: Vec<f32>,
    pub bad_frames: Vec<u32>,
    pub nframes: usize,
    pub nvectors: usize,
    pub ngroups: usize,
    pub nlags: usize,
}

/// What `Engine::structure_factor` returns: rho [frame][group][m][re, im] and rho_mean [group][m][re, im] (empty unless asked
/// for), frame_ok [frame], sab [pair a <= b, a-major][m], shell [pair][shell] (NaN for a shell without a member) and the members
/// of every shell over the block; m is the lattice index (h (2K + 1) + (k + K)) (2L + 1) + (l + L).
#[derive(Debug, Clone, Default)]
pub struct StructureFactor {
    pub rho: Vec<f32>,
    pub frame_ok: Vec<u32>,
    pub rho_mean: Vec<f32>,
    pub sab: Vec<f32>,
    pub shell: Vec<f32>,
    pub shell_count: Vec<u64>,
    pub nframes: usize,
    pub ngroups: usize,
    pub npairs: usize,
    pub nq: usize,
    pub nshells: usize,
}

/// What `Engine::min_distances` returns: dist [frame] and pair [frame][i, j]; atom1, near1 [frame][atom of set 1]; atom2
/// [frame][atom of set 2]; mat [frame][group of set 1][group of set 2] and its mean, minimum and count below the cutoff over the
/// valid frames; frame_ok [frame] and the number of valid frames.  Empty where not asked for.
#[derive(Debug, Clone, Default)]
pub struct MinDistances {
    pub dist: Vec<f32>,
    pub pair: Vec<u64>,
    pub atom1: Vec<f32>,
    pub near1: Vec<u64>,
    pub atom2: Vec<f32>,
    pub mat: Vec<f32>,
    pub mat_mean: Vec<f64>,
    pub mat_min: Vec<f32>,
    pub mat_freq: Vec<u32>,
    pub frame_ok: Vec<u32>,
    pub nvalid: u64,
    pub nframes: usize,
    pub n1: usize,
    pub n2: usize,
    pub ngroups1: usize,
    pub ngroups2: usize,
}

/// What `Engine::fluctuations` returns: the mean structure, the per-atom RMSF, the 3n x 3n covariance row by row (empty unless
/// asked for) and per frame {R column-major, t, rmsd} (empty unless asked for).
#[derive(Debug, Clone, Default)]
pub struct Fluctuations {
    pub mean: Vec<[f32; 3]>,
    pub rmsf: Vec<f32>,
    pub cov: Vec<f32>,
    pub fit: Vec<[f32; 13]>,
}

/// What one frame of a streamed fit returns: `fit_transform` (measure.rs:507-522) as (R column-major, t), and RMSD / centre of
/// mass / gyration of the fitted selection.
#[derive(Clone, Copy, Debug)]
pub struct FitRecord {
    pub r: [f32; 9],
    pub t: [f32; 3],
    pub rmsd: f32,
    pub com: [f32; 3],
    pub gyration: f32,
}

/// The per-frame fit loop of `benches/comparison_small.rs:14-25` for States in host memory (`analysis_task.rs:245-252` hands
/// them to the task one by one), at the rate the SELECTION crosses the link: `molar_hip_fit_stream_*`.  Up to three frames in
/// flight: `let t1 = fs.begin(&mut next, false)?; let rec = fs.end(t0)?;`.
pub struct FitStream<'e> {
    engine: &'e Engine,
    handle: *mut types::MolarHipFitStream,
    natoms: usize,
}

impl<'e> FitStream<'e> {
    /// `index` / `ref_index`: the selection in the frames and in the reference (None = all atoms); `masses`: the topology's
    /// column; `reference`: the frame fitted onto.
    pub fn new(
        engine: &'e Engine, natoms: usize, index: Option<&[usize]>, masses: &[f32], reference: &[[f32; 3]], ref_index: Option<&[usize]>,
        host_threads: i32,
    ) -> Result<Self, EngineError> {
        check_index(index, natoms, "FitStream::new (selection)")?;
        check_index(ref_index, reference.len(), "FitStream::new (reference)")?;
        check_column(masses.len(), natoms, "FitStream::new: masses")?;
        let (ip, n) = idx_ptr(index);
        let (rp, rn) = idx_ptr(ref_index);
        if index.is_some() != ref_index.is_some() || n != rn {
            return Err(EngineError::Sizes("FitStream::new: the two selections differ in size".into()));
        }
        let mut handle = std::ptr::null_mut();
        engine.plugin.check(unsafe {
            (engine.plugin.fns.fit_stream_create)(engine.ctx, natoms, ip, n, masses.as_ptr(), reference.as_ptr() as *const f32, reference.len(), rp,
                                                  host_threads, &mut handle)
        })?;
        Ok(FitStream { engine, handle, natoms })
    }

    /// Enqueues one frame.  With `apply` the fitted selection is written into `coords` by `end` (`Modify::apply_transform`,
    /// modify.rs:32-36): the borrow the ticket stands for must stay alive and untouched until then - hence `unsafe`.
    ///
    /// # Safety
    /// `coords` must outlive the matching `end` call and must not be read or written in between.
    pub unsafe fn begin(&mut self, coords: &mut [[f32; 3]], apply: bool) -> Result<i32, EngineError> {
        if coords.len() != self.natoms {
            return Err(EngineError::Sizes(format!("FitStream::begin: frame of {} atoms, stream built for {}", coords.len(), self.natoms)));
        }
        let mut ticket = -1i32;
        self.engine.plugin.check(unsafe { (self.engine.plugin.fns.fit_stream_begin)(self.handle, coords.as_mut_ptr() as *mut f32, apply as i32, &mut ticket) })?;
        Ok(ticket)
    }

    pub fn end(&mut self, ticket: i32) -> Result<FitRecord, EngineError> {
        let mut rec = FitRecord { r: [0.0; 9], t: [0.0; 3], rmsd: 0.0, com: [0.0; 3], gyration: 0.0 };
        self.engine.plugin.check(unsafe {
            (self.engine.plugin.fns.fit_stream_end)(self.handle, ticket, &mut rec.rmsd, rec.r.as_mut_ptr(), rec.t.as_mut_ptr(), rec.com.as_mut_ptr(),
                                                   &mut rec.gyration)
        })?;
        Ok(rec)
    }
}

impl Drop for FitStream<'_> {
    fn drop(&mut self) {
        unsafe { (self.engine.plugin.fns.fit_stream_destroy)(self.handle) }
    }
}

/// The remaining entry points (histogram-fused search, resident/pipelined search, batched fits, membrane smoothing,
/// lipid order, XTC reader, PeriodicBox helpers) are reachable through `Engine::raw()`; they take the same pointer/size
/// pairs and follow the count-then-fill convention documented in `include/molar_hip.h`.
impl Engine {
    pub fn raw(&self) -> (&MolarHipFns, *mut MolarHipCtx) {
        (&self.plugin.fns, self.ctx)
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Bilayer frames: `Membrane::compute` (molar_membrane/src/lib.rs:410-454) as one chained call per frame
// (molar_hip_membrane_frame_begin / _end / _fetch), the Rust side of `MembraneFrames` in include/molar_hip.hpp.

/// Index lists of a bilayer, as `Membrane::new` collects them per lipid (lib.rs:120-177): whole lipids, the three marker
/// sub-selections (head, mid, tail end) per lipid, and the tails' carbons with their bond orders.
pub struct MembraneLayout<'a> {
    pub natoms: usize,
    pub lipid_idx: &'a [usize],
    pub lipid_offsets: &'a [usize],
    pub marker_idx: &'a [usize],
    pub marker_offsets: &'a [usize],
    pub masses: &'a [f32],
    pub tail_idx: &'a [usize],
    pub tail_offsets: &'a [usize],
    pub tail_lipid: &'a [u32],
    pub tail_bonds: &'a [u8],
    pub cutoff: f32,
    pub order_type: i32,
    pub max_smooth_iter: i32,
    pub unwrap: bool,
    pub global_normal: Option<[f32; 3]>,
}

/// Per-lipid results of one frame copied to the host (the arrays `LipidGroup::frame_update` reads, lipid_group.rs).
pub struct MembraneFrame {
    pub valid: Vec<u8>,
    pub normals: Vec<[f32; 3]>,
    pub mean_curv: Vec<f32>,
    pub gauss_curv: Vec<f32>,
    pub area: Vec<f32>,
    pub nvert: Vec<u32>,
    pub neib_ids: Vec<u64>,
    pub patch_offsets: Vec<u64>,
    pub order: Vec<f32>,
}

/// Two frames in flight on one engine: `push(frame k+1)` returns the results of frame k.
pub struct MembraneFrames<'e> {
    engine: &'e Engine,
    plan: *mut MolarHipMembranePlan,
    nlipids: usize,
    natoms: usize,
    pending: Option<i32>,
}

impl<'e> MembraneFrames<'e> {
    pub fn new(engine: &'e Engine, l: &MembraneLayout) -> Result<Self, EngineError> {
        let k = l.lipid_offsets.len().saturating_sub(1);
        check_offsets(l.lipid_offsets, l.lipid_idx.len(), "MembraneFrames: lipids")?;
        check_offsets(l.marker_offsets, l.marker_idx.len(), "MembraneFrames: markers")?;
        check_offsets(l.tail_offsets, l.tail_idx.len(), "MembraneFrames: tails")?;
        check_index(Some(l.lipid_idx), l.natoms, "MembraneFrames: lipids")?;
        check_index(Some(l.marker_idx), l.natoms, "MembraneFrames: markers")?;
        check_index(Some(l.tail_idx), l.natoms, "MembraneFrames: tails")?;
        check_column(l.masses.len(), l.natoms, "MembraneFrames: masses")?;
        let ntails = l.tail_offsets.len().saturating_sub(1);
        if l.marker_offsets.len() != 3 * k + 1 || l.tail_lipid.len() != ntails || l.tail_bonds.len() + ntails < l.tail_idx.len() {
            return Err(EngineError::Sizes("MembraneFrames: three marker selections per lipid, one lipid and n-1 bond orders per tail".into()));
        }
        let d = MolarHipMembraneDesc {
            natoms: l.natoms,
            nlipids: k,
            lipid_idx: l.lipid_idx.as_ptr() as *const u64,
            lipid_offsets: l.lipid_offsets.as_ptr() as *const u64,
            marker_idx: l.marker_idx.as_ptr() as *const u64,
            marker_offsets: l.marker_offsets.as_ptr() as *const u64,
            masses: l.masses.as_ptr(),
            ntails,
            tail_idx: l.tail_idx.as_ptr() as *const u64,
            tail_offsets: l.tail_offsets.as_ptr() as *const u64,
            tail_lipid: l.tail_lipid.as_ptr(),
            tail_bonds: l.tail_bonds.as_ptr(),
            cutoff: l.cutoff,
            order_type: l.order_type,
            max_smooth_iter: l.max_smooth_iter,
            unwrap: l.unwrap as i32,
            use_global_normal: l.global_normal.is_some() as i32,
            global_normal: l.global_normal.unwrap_or([0.0; 3]),
        };
        let mut plan = std::ptr::null_mut();
        engine.plugin.check(unsafe { (engine.plugin.fns.membrane_plan_create)(engine.ctx, &d, &mut plan) })?;
        Ok(MembraneFrames { engine, plan, nlipids: k, natoms: l.natoms, pending: None })
    }

    /// `reset_valid_lipids` (lib.rs:269-273) with `None`, or the caller's flags; ends the frame in flight first.
    pub fn set_valid(&mut self, valid: Option<&[u8]>) -> Result<Option<MembraneFrame>, EngineError> {
        let last = self.finish()?;
        if let Some(v) = valid {
            if v.len() != self.nlipids {
                return Err(EngineError::Sizes(format!("set_valid: {} flags for {} lipids", v.len(), self.nlipids)));
            }
        }
        let p = valid.map_or(std::ptr::null(), |v| v.as_ptr());
        self.engine.plugin.check(unsafe { (self.engine.plugin.fns.membrane_plan_set_valid)(self.plan, p) })?;
        Ok(last)
    }

    /// `n_shells_patch` / `n_shells_smoothing` of `MembraneOptions` (lib.rs:53-85) for the frames pushed from now on
    /// (0, 0: none); ends the frame in flight first.
    pub fn set_shells(&mut self, n_shells_patch: usize, n_shells_smoothing: usize) -> Result<Option<MembraneFrame>, EngineError> {
        let last = self.finish()?;
        self.engine.plugin.check(unsafe { (self.engine.plugin.fns.membrane_plan_set_shells)(self.plan, n_shells_patch, n_shells_smoothing) })?;
        Ok(last)
    }

    /// Enqueue one frame (coordinates are unwrapped in place) and collect the frame pushed before it.
    pub fn push(&mut self, coords: &mut [[f32; 3]], box9: &[f32; 9]) -> Result<Option<MembraneFrame>, EngineError> {
        if coords.len() != self.natoms {
            return Err(EngineError::Sizes(format!("push: {} atoms, the layout was made for {}", coords.len(), self.natoms)));
        }
        let mut t = -1i32;
        self.engine.plugin.check(unsafe {
            (self.engine.plugin.fns.membrane_frame_begin)(self.plan, coords.as_mut_ptr() as *mut f32, box9.as_ptr(), &mut t)
        })?;
        let last = self.finish()?;
        self.pending = Some(t);
        Ok(last)
    }

    /// Collect the frame in flight, if any.
    pub fn finish(&mut self) -> Result<Option<MembraneFrame>, EngineError> {
        let Some(t) = self.pending.take() else { return Ok(None) };
        let f = &self.engine.plugin.fns;
        let mut v: MolarHipMembraneView = unsafe { std::mem::zeroed() };
        self.engine.plugin.check(unsafe { (f.membrane_frame_end)(self.plan, t, &mut v) })?;
        let k = self.nlipids;
        let mut r = MembraneFrame {
            valid: vec![0; k],
            normals: vec![[0.0; 3]; k],
            mean_curv: vec![0.0; k],
            gauss_curv: vec![0.0; k],
            area: vec![0.0; k],
            nvert: vec![0; k],
            neib_ids: vec![0; v.patch_entries + 4 * k],
            patch_offsets: vec![0; k + 1],
            order: vec![0.0; v.norder],
        };
        let mut o: MolarHipMembraneOut = unsafe { std::mem::zeroed() };
        o.valid = r.valid.as_mut_ptr();
        o.normals = r.normals.as_mut_ptr() as *mut f32;
        o.mean_curv = r.mean_curv.as_mut_ptr();
        o.gauss_curv = r.gauss_curv.as_mut_ptr();
        o.area = r.area.as_mut_ptr();
        o.nvert = r.nvert.as_mut_ptr();
        o.neib_ids = r.neib_ids.as_mut_ptr();
        o.patch_offsets = r.patch_offsets.as_mut_ptr();
        o.order = r.order.as_mut_ptr();
        self.engine.plugin.check(unsafe { (f.membrane_frame_fetch)(self.plan, t, &o) })?;
        Ok(Some(r))
    }
}

impl Drop for MembraneFrames<'_> {
    fn drop(&mut self) {
        unsafe { (self.engine.plugin.fns.membrane_plan_destroy)(self.plan) }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Frame-parallel driver for one node with several GPUs - the Rust side of `AnalysisTask::run_sharded` in
// include/molar_hip.hpp.  MolAR's `AnalysisTask::run` (analysis_task.rs:202-267) is a serial loop over frames whose
// body does not depend on earlier frames for the analyses on this path (search, fit/RMSD, Measure); frames therefore
// shard embarrassingly: one engine context and one task instance per device, contiguous blocks of frames dealt
// round-robin, no exchange until the end, then an integer reduction (`merge`) in worker order.

/// Number of GPUs the engine sees (`molar_hip_device_count`); 0 when the library or a GPU is missing.
pub fn device_count() -> usize {
    match Plugin::get_cached() {
        Ok(p) => unsafe { (p.fns.device_count)() }.max(0) as usize,
        Err(_) => 0,
    }
}

/// What a frame-parallel analysis provides.  `new` plays the role of `AnalysisTask::new`: every instance is built on the
/// FIRST consumed frame of the run (so a reference structure taken there is the same on every device); only the worker
/// that owns frame 0 also processes it.
pub trait ShardedTask: Send + Sized {
    type Frame: Send + Sync + Clone;
    fn new(engine: &Engine, first: &Self::Frame) -> Result<Self, EngineError>;
    /// `frame_index` is the position of the frame among the consumed frames of the whole run: per-frame results are
    /// tagged with it and put back in order by `merge`.
    fn process_frame(&mut self, engine: &Engine, frame_index: usize, frame: Self::Frame) -> Result<(), EngineError>;
    /// Folds another worker's instance into this one: integer accumulators (histogram bins, pair counts) add, per-frame
    /// series are concatenated and sorted by frame index.
    fn merge(&mut self, other: Self);
}

/// Runs `frames` (already windowed by -b/-e/--skip: the iterator is what `AnalysisTask::run` would consume, read by the
/// calling thread) through one worker per entry of `devices`, in blocks of `block` consecutive frames.  Returns the merged
/// instance and the number of frames consumed; `None` if the iterator was empty.
pub fn run_sharded<T, I>(devices: &[i32], block: usize, frames: I) -> Result<Option<(T, usize)>, EngineError>
where
    T: ShardedTask,
    I: Iterator<Item = T::Frame>,
{
    use std::sync::mpsc::sync_channel;
    if devices.is_empty() {
        return Err(EngineError::Sizes("run_sharded: no devices".into()));
    }
    let block = block.max(1);
    let mut frames = frames.enumerate().peekable();
    let first = match frames.peek() {
        Some((_, f)) => f.clone(),
        None => return Ok(None),
    };
    let first = &first;
    std::thread::scope(|scope| {
        let mut senders = Vec::with_capacity(devices.len());
        let mut handles = Vec::with_capacity(devices.len());
        for &dev in devices {
            let (tx, rx) = sync_channel::<(usize, T::Frame)>(2 * block + 2);
            senders.push(tx);
            handles.push(scope.spawn(move || -> Result<Option<(T, usize)>, EngineError> {
                let engine = Engine::new(dev)?;
                let mut task: Option<T> = None;
                let mut done = 0usize;
                for (index, frame) in rx {
                    if task.is_none() {
                        task = Some(T::new(&engine, first)?);
                    }
                    task.as_mut().unwrap().process_frame(&engine, index, frame)?;
                    done += 1;
                }
                Ok(task.map(|t| (t, done)))
            }));
        }
        for (index, frame) in frames {
            // a worker that failed has dropped its receiver: stop feeding, its error is collected below
            if senders[(index / block) % devices.len()].send((index, frame)).is_err() {
                break;
            }
        }
        drop(senders);
        let mut merged: Option<(T, usize)> = None;
        let mut failure = None;
        for h in handles {
            match h.join().unwrap_or_else(|_| Err(EngineError::Other("run_sharded: a worker panicked".into()))) {
                Ok(Some((t, n))) => match merged.as_mut() {
                    Some((head, total)) => {
                        head.merge(t);
                        *total += n;
                    }
                    None => merged = Some((t, n)),
                },
                Ok(None) => {}
                Err(e) => failure = failure.or(Some(e)),
            }
        }
        match failure {
            Some(e) => Err(e),
            None => Ok(merged),
        }
    })
}

/// The same with one reader PER WORKER (`run_sharded_own_readers` in include/molar_hip.hpp): `nframes` consumed frames are
/// known up front (an indexed trajectory: `FileHandler` random access, io.rs:691-760), worker `w` takes the contiguous block
/// `[w * ceil(n / W), ...)` and gets its frames from `open(first_index)` - its own reader, positioned at the block's first
/// consumed frame (with `--skip` the reader yields consumed frames only).  No producer thread, no channel: a single reader
/// decodes ~460 frames/s of 250k atoms per host thread, eight GPUs binning 4 k frames/s each would wait for it.  `first` is the
/// first consumed frame of the run, on which every instance is built.  Returns the merged instance and the frames consumed.
pub fn run_sharded_readers<T, O, R>(devices: &[i32], nframes: usize, first: &T::Frame, open: O) -> Result<Option<(T, usize)>, EngineError>
where
    T: ShardedTask,
    O: Fn(usize) -> Result<R, EngineError> + Sync,
    R: Iterator<Item = T::Frame>,
{
    if devices.is_empty() {
        return Err(EngineError::Sizes("run_sharded_readers: no devices".into()));
    }
    if nframes == 0 {
        return Ok(None);
    }
    let per = (nframes + devices.len() - 1) / devices.len();
    let open = &open;
    std::thread::scope(|scope| {
        let mut handles = Vec::with_capacity(devices.len());
        for (w, &dev) in devices.iter().enumerate() {
            let (lo, hi) = ((w * per).min(nframes), ((w + 1) * per).min(nframes));
            handles.push(scope.spawn(move || -> Result<Option<(T, usize)>, EngineError> {
                if lo == hi {
                    return Ok(None);
                }
                let engine = Engine::new(dev)?;
                let mut task = T::new(&engine, first)?;
                let mut done = 0usize;
                for (k, frame) in open(lo)?.take(hi - lo).enumerate() {
                    task.process_frame(&engine, lo + k, frame)?;
                    done += 1;
                }
                if done != hi - lo {
                    return Err(EngineError::Other(format!("run_sharded_readers: the reader of frames {lo}..{hi} ended after {done}")));
                }
                Ok(Some((task, done)))
            }));
        }
        let mut merged: Option<(T, usize)> = None;
        let mut failure = None;
        for h in handles {
            match h.join().unwrap_or_else(|_| Err(EngineError::Other("run_sharded_readers: a worker panicked".into()))) {
                Ok(Some((t, n))) => match merged.as_mut() {
                    Some((head, total)) => {
                        head.merge(t);
                        *total += n;
                    }
                    None => merged = Some((t, n)),
                },
                Ok(None) => {}
                Err(e) => failure = failure.or(Some(e)),
            }
        }
        match failure {
            Some(e) => Err(e),
            None => Ok(merged),
        }
    })
}
