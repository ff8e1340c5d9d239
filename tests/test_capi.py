"""CPU: the HIP library builds for gfx950, loads, and exports every symbol include/pxsht.h declares.
No compute call is made (there is no GPU here)."""
import os, re, ctypes
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

def _header_symbols():
	txt = open(os.path.join(ROOT, "include", "pxsht.h")).read()
	txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
	return sorted(set(re.findall(r"\b(px[sfam]_[a-z0-9_]+)\s*\(", txt)))

def test_header_declares_expected_entry_points():
	syms = _header_symbols()
	for s in ["pxs_plan_rings", "pxs_plan_grid2d", "pxs_plan_destroy", "pxs_synthesis", "pxs_analysis",
			"pxs_gridweights", "pxf_fft_nd", "pxs_last_error"]:
		assert s in syms

def test_hip_library_builds_loads_and_exports():
	from pixell_amd import _build
	lib = _build.build()
	assert os.path.exists(lib)
	h = ctypes.CDLL(lib)
	for s in _header_symbols():
		assert hasattr(h, s), "libpxsht.so does not export %s" % s
	h.pxs_version.restype = ctypes.c_char_p
	assert b"gfx950" in h.pxs_version()

def test_a_translation_unit_really_compiles_for_gfx950(tmp_path):
	"""not an mtime check: hipcc cross-compiles one kernel file from scratch and the object carries gfx950 code"""
	import subprocess
	from pixell_amd import _build
	obj = _build.compile_one(os.path.join(_build.CSRC, "flatsky.hip"), str(tmp_path/"flatsky.o"))
	assert os.path.getsize(obj) > 10000
	blob = open(obj, "rb").read()
	assert b"gfx950" in blob and b"pxm_ps2d" in blob

def test_loader_export_list_matches_header():
	from pixell_amd import _lib
	assert sorted(_lib.EXPORTS) == _header_symbols()

def test_product_loader_has_no_cpu_fallback(monkeypatch, tmp_path):
	"""the loader raises when the HIP library is missing (it never substitutes the oracle or the simulator)"""
	from pixell_amd import _lib
	monkeypatch.setattr(_lib, "_lib", None)
	monkeypatch.setattr(_lib, "lib_path", lambda: str(tmp_path/"missing.so"))
	with pytest.raises(ImportError):
		_lib.load()

def test_product_package_does_not_import_oracle():
	import glob
	for f in glob.glob(os.path.join(ROOT, "pixell_amd", "*.py")):
		src = open(f).read()
		assert "import oracle" not in src and "from oracle" not in src, f


def test_default_build_carries_no_lab_switches():
	"""The switches that turn parts of a transform OFF (timing experiments: wrong results) and the experimental kernel families exist in
	lab builds only (-DPXS_LAB, tools/build_variants.sh): the library __graft_entry__.build() makes must not even contain their names."""
	from pixell_amd import _build
	blob = open(_build.build(), "rb").read()
	for name in (b"PXS_CH_NOFFT", b"PXS_CH_NOTW", b"PXS_CH_NOPH", b"PXS_FFT_DEBUG_NOPASS", b"PXS_CHAIN_V2", b"PXS_CH2_", b"PXS_SYN_SHARE", b"chain2_kernel", b"leg_syn_s0b",
			b"PXS_FFT_NT", b"PXS_FFT_ODDFIRST", b"PXS_FFT_ALIGN8", b"PXS_FFT_RADICES", b"PXS_FFT_COMP", b"PXS_FFT_PTS", b"PXS_FFT_LINEPAD", b"PXS_BLUESTEIN_MINPRIME", b"PXS_TL_"):
		assert name not in blob, name

def test_docs_agree_with_the_header():
	"""the entry-point count quoted in INTEGRATION.md / DESIGN.md / README.md is the number of declarations in include/pxsht.h,
	and every declared symbol is in the loader's export list"""
	import re
	from pixell_amd import _lib
	hdr = open(os.path.join(ROOT, "include", "pxsht.h")).read()
	names = re.findall(r"^(?:int|void|int64_t|const char\*)\s+(px[a-z]_\w+)\s*\(", hdr, re.M)
	assert len(names) == len(set(names)) and set(names) == set(_lib.EXPORTS), sorted(set(names) ^ set(_lib.EXPORTS))
	for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
		txt = open(os.path.join(ROOT, doc)).read()
		counts = set(int(n) for n in re.findall(r"(\d+) entry points", txt))
		assert counts == {len(names)}, (doc, counts, len(names))
