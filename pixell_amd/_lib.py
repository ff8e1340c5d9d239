"""ctypes loader of libpxsht.so (the HIP kernels behind include/pxsht.h).

The product path has NO CPU fallback: if the library is missing or cannot be loaded this
module raises.  There is no switch in here that selects anything but pixell_amd/libpxsht.so: the
CPU test-suite points `lib_path` at its simulator build itself (tests/conftest.py), and such a
build says what it is in pxs_version() (`is_hostsim`)."""
import ctypes, os

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None
_is_hostsim = False

class PxsError(RuntimeError):
	def __init__(self, code, msg):
		RuntimeError.__init__(self, "libpxsht error %d: %s" % (code, msg))
		self.code = code

def _declare(lib):
	c = ctypes
	vp, i32, i64, dbl = c.c_void_p, c.c_int, c.c_int64, c.c_double
	lib.pxs_last_error.restype = c.c_char_p
	lib.pxs_version.restype = c.c_char_p
	lib.pxs_plan_rings.argtypes = [c.POINTER(vp), i32, vp, vp, vp, vp, i64, i32, i32, vp, i64, i32]
	lib.pxs_plan_grid2d.argtypes = [c.POINTER(vp), c.c_char_p, i32, i32, dbl, i32, i32, i32, i32, vp, i64, i32]
	lib.pxs_plan_points.argtypes = [c.POINTER(vp), vp, i64, vp, dbl, i32, vp]
	lib.pxs_plan_destroy.argtypes = [vp]; lib.pxs_plan_destroy.restype = None
	lib.pxs_synthesis.argtypes = [vp, i32, i32, i32, i32, vp, i32, i64, i64, vp, i32, i64, i64, vp]
	lib.pxs_analysis.argtypes = [vp, i32, i32, i32, vp, i32, i64, i64, vp, i32, i64, i64, vp]
	lib.pxs_gridweights.argtypes = [c.c_char_p, i32, vp]
	lib.pxs_grid_maxlmax.argtypes = [c.c_char_p, i32]
	lib.pxs_plan_info.argtypes = [vp, c.POINTER(i32), c.POINTER(i32), c.POINTER(i64)]
	lib.pxs_plan_option.argtypes = [vp, c.c_char_p, i64]
	lib.pxs_plan_query.argtypes = [vp, c.c_char_p, c.POINTER(i64)]      # names: include/pxsht.h ("analysis_form", "ncc_circle", "ducc_ncc_circle", "theta_line", "chain_stages", "chain_static", "chain_static_table", "passes_<seam>": plan may be NULL for "passes_fft")
	lib.pxs_profile.argtypes = [vp, i32]; lib.pxs_profile_read.argtypes = [vp, vp, vp, i32]; lib.pxs_profile_flops.argtypes = [vp, vp, i32]
	lib.pxs_debug_theta_plan.argtypes = [i64, i32, vp]; lib.pxs_debug_chain.argtypes = [vp, i32, i32, i32, i32, vp]
	lib.pxs_memory.argtypes = [i32, vp]
	lib.pxa_alm2cl.argtypes = [i32, i32, vp, i64, vp, vp, i32, vp, i32, i32, vp]
	lib.pxa_lmatmul.argtypes = [i32, i32, i32, i32, vp, i64, vp, i64, vp, i64, i32, vp, i32, i32, vp]
	lib.pxa_rotate_alm.argtypes = [i32, i32, vp, i64, vp, i64, i32, dbl, dbl, dbl, i32, vp]
	lib.pxa_bank_split.argtypes = [i32, vp, vp, vp, vp, i32, i32, i32, vp, i64, vp, i64, i32, vp, i32, i32, vp]
	lib.pxa_bank_merge.argtypes = [i32, vp, vp, vp, vp, i32, i32, i32, vp, i64, vp, i64, i32, vp, i32, i32, i32, vp]
	f64 = ctypes.c_double
	lib.pxm_rotate_queb.argtypes = [i32, i32, vp, vp, i32, i32, vp, vp, i32, i32, vp]
	lib.pxm_ps2d.argtypes = [i64, vp, vp, i32, vp, i32, i32, vp]
	lib.pxm_lbin.argtypes = [i32, i32, vp, vp, f64, i32, vp, i32, vp, vp, vp, i32, vp]
	lib.pxm_bin_index.argtypes = [i64, vp, i32, vp, i32, vp, i32, vp]
	lib.pxm_mul_axis.argtypes = [i64, i64, i64, vp, i32, vp, i32, vp]
	lib.pxm_deflect.argtypes = [i64, i32, i32, dbl, dbl, dbl, dbl, vp, i32, vp, i32, i64, i32, vp, vp, i32, vp]
	lib.pxm_rotate_pol.argtypes = [i64, i32, vp, vp, i64, i32, vp, i32, i32, vp]
	lib.pxm_plan_map_points.argtypes = [c.POINTER(vp), i32, i32, i32, i64, vp, dbl, i32, vp]
	lib.pxm_map_points.argtypes = [vp, i32, vp, i32, i64, vp, i32, i64, vp]
	lib.pxm_modulate.argtypes = [i64, i32, vp, i32, i64, vp, c.c_uint64, i32, i32, dbl, dbl, dbl, i32, vp]
	lib.pxm_sim_objects.argtypes = [i32, i32, dbl, dbl, dbl, dbl, vp, i32, i32, i64, i64, vp, vp, vp, i64, vp, i32, vp, i64, vp, vp, vp, i32, dbl, dbl, i32, i32, i32, vp]
	lib.pxm_radial_sum.argtypes = [i32, i32, dbl, dbl, dbl, dbl, vp, i32, i32, i64, i64, vp, vp, i32, vp, dbl, i32, vp, i32, vp]
	lib.pxm_find_edges.argtypes = [i32, i32, vp, i32, vp, i64, c.POINTER(i64), i32, vp]
	lib.pxm_distance_from.argtypes = [i32, i32, dbl, dbl, dbl, dbl, i64, vp, vp, vp, dbl, vp, vp, i32, vp, vp, i32, vp]
	lib.pxm_spline_filter.argtypes = [i32, i32, i32, vp, i32, i64, vp, vp, i32, i32, vp]
	lib.pxm_interpol.argtypes = [i32, i32, i32, vp, i32, i64, i64, vp, i32, i32, dbl, dbl, dbl, dbl, dbl, dbl, dbl, dbl, i32, i32, dbl, vp, i32, vp]
	lib.pxm_spline_filter_axes.argtypes = [i32, i32, i32, vp, i32, i64, vp, vp, i32, i32, i32, vp]
	lib.pxm_thumbnails.argtypes = [i32, i32, i32, vp, i32, i64, dbl, dbl, dbl, dbl, dbl, dbl, dbl, dbl, i64, vp, i32, i32, i32, dbl, dbl, dbl, dbl,
		i32, i32, i32, dbl, i32, i32, i32, vp, i32, vp]
	lib.pxm_healpix_index.argtypes = [i32, i64, i64, vp, vp, vp, vp, vp, i32, vp]
	lib.pxm_healpix_interp.argtypes = [i64, i32, vp, i32, i64, i64, vp, vp, i32, vp, i32, vp]
	lib.pxm_map2healpix.argtypes = [i32, i32, i32, vp, i32, i64, dbl, dbl, dbl, dbl, dbl, dbl, dbl, dbl, i32, i32, i32, dbl, i64, i64, i64, vp, i32, vp, dbl, vp, i32, i64, i32, vp]
	lib.pxm_healpix2map.argtypes = [i32, i64, vp, i32, i64, i32, i32, dbl, dbl, dbl, dbl, i32, vp, i32, vp, vp, vp, i32, vp]
	lib.pxm_label.argtypes = [i32, i32, vp, i32, i32, vp, c.POINTER(i64), i32, vp]
	lib.pxm_label_stats.argtypes = [i32, i32, vp, i64, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp]
	lib.pxm_solve_mapsys.argtypes = [i32, i64, vp, vp, vp, vp, i32, i32, vp]
	lib.pxf_fft_nd.argtypes = [i32, vp, vp, vp, i32, vp, i32, i32, dbl, i32, i32, vp, vp, i32, vp]
	lib.pxf_fft_supported.argtypes = [i64]
	lib.pxf_fft_good_size.argtypes = [i64]; lib.pxf_fft_good_size.restype = i64
	for name in ["pxs_plan_rings", "pxs_plan_grid2d", "pxs_plan_points", "pxs_synthesis", "pxs_analysis", "pxs_gridweights",
			"pxs_grid_maxlmax", "pxs_plan_info", "pxs_plan_option", "pxs_plan_query", "pxf_fft_nd", "pxf_fft_supported", "pxs_profile", "pxs_profile_read", "pxs_profile_flops", "pxs_debug_theta_plan", "pxs_debug_chain", "pxs_memory", "pxa_alm2cl", "pxa_lmatmul", "pxa_rotate_alm", "pxa_bank_split", "pxa_bank_merge", "pxm_rotate_queb", "pxm_ps2d", "pxm_lbin", "pxm_bin_index", "pxm_mul_axis", "pxm_deflect", "pxm_rotate_pol", "pxm_plan_map_points", "pxm_map_points", "pxm_modulate", "pxm_sim_objects", "pxm_radial_sum", "pxm_find_edges", "pxm_distance_from", "pxm_spline_filter", "pxm_interpol", "pxm_spline_filter_axes", "pxm_thumbnails", "pxm_healpix_index", "pxm_healpix_interp", "pxm_map2healpix", "pxm_healpix2map", "pxm_label", "pxm_label_stats", "pxm_solve_mapsys"]:
		getattr(lib, name).restype = i32
	return lib

EXPORTS = ["pxs_plan_rings", "pxs_plan_grid2d", "pxs_plan_points", "pxs_plan_destroy", "pxs_synthesis", "pxs_analysis",
	"pxs_gridweights", "pxs_grid_maxlmax", "pxs_plan_info", "pxs_plan_option", "pxs_plan_query", "pxf_fft_nd", "pxf_fft_supported",
	"pxf_fft_good_size", "pxs_last_error", "pxs_version", "pxs_profile", "pxs_profile_read", "pxs_profile_flops", "pxs_debug_theta_plan", "pxs_debug_chain", "pxs_memory", "pxa_alm2cl", "pxa_lmatmul", "pxa_rotate_alm", "pxa_bank_split", "pxa_bank_merge", "pxm_rotate_queb", "pxm_ps2d", "pxm_lbin", "pxm_bin_index", "pxm_mul_axis", "pxm_deflect", "pxm_rotate_pol", "pxm_plan_map_points", "pxm_map_points", "pxm_modulate", "pxm_sim_objects", "pxm_radial_sum", "pxm_find_edges", "pxm_distance_from", "pxm_spline_filter", "pxm_interpol", "pxm_spline_filter_axes", "pxm_thumbnails", "pxm_healpix_index", "pxm_healpix_interp", "pxm_map2healpix", "pxm_healpix2map", "pxm_label", "pxm_label_stats", "pxm_solve_mapsys"]

def lib_path():
	# PIXELL_AMD_LIB: another build of the same library (kernel A/B experiments, tools/build_variants.sh, tools/gpu_v2lab.sh, tools/gpu_leg_ab.sh)
	return os.environ.get("PIXELL_AMD_LIB") or os.path.join(HERE, "libpxsht.so")

def load():
	"""Return the loaded library, loading it on first use.  Raises if it is absent."""
	global _lib, _is_hostsim
	if _lib is not None: return _lib
	path = lib_path()
	if not os.path.exists(path):
		raise ImportError("pixell_amd: %s not found. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
			"(hipcc --offload-arch=gfx950). There is no CPU fallback." % path)
	# torch ships its own libamdhip64: let it be the HIP runtime of the process.  Loading libpxsht.so (which pulls in
	# /opt/rocm's runtime) before torch left two runtimes in one process and hipSetDevice then reported no device.
	try: import torch  # noqa: F401
	except ImportError: pass
	lib = _declare(ctypes.CDLL(path))
	_is_hostsim = b"HOSTSIM" in lib.pxs_version()      # a g++ build of the kernel sources (tests/hostsim): host pointers, no streams
	_lib = lib
	return _lib

def is_hostsim():
	load(); return _is_hostsim

def check(code):
	if code != 0:
		raise PxsError(code, load().pxs_last_error().decode("utf-8", "replace"))
