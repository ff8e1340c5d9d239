"""Connected components of a mask and reductions over label maps on the device: what the reference's analysis.py takes from
scipy.ndimage (label, center_of_mass, maximum, ..., analysis.py:553-564).

label numbers the connected regions of a mask (pxm_label, csrc/label.hip); stats gives, in one call, the count, bounding box, weighted sums,
maximum and minimum with their positions of every label of a label map (pxm_label_stats), which need not come from label: grown labels
(enmap.labeled_distance_transform) or painted ones do as well.  center_of_mass, maximum, minimum, maximum_position, minimum_position,
sum_labels and find_objects read that table in scipy.ndimage's shapes.  Numpy in gives numpy arrays / ndmaps out; CUDA tensors or a dmap
in give tensors / a dmap out on that device, and no map goes to the host.

Where this differs from the reference on purpose: the labels are scipy's bit for bit (components in ascending order of
their lowest flat pixel index), `wrap` is ours, the sums are accumulated in arrival order (repeatable to rounding, not bit for bit), and
the readers return arrays ([nindex, 2] positions) where scipy returns lists of tuples."""
import ctypes
import numpy as np
from . import enmap, _lib, _arrays as A

TILE = 16      # the labelling kernel's tile: components that cross a multiple of TILE in y or x are joined by its second step
MAX_PIX = 2**31

class LabelStats:
	"""The per-label table of stats(): arrays [nlabel], entry l-1 for label l.  count (int64); ymin, ymax, xmin, xmax (int32, the bounding
	box, inclusive); sum_w, sum_wy, sum_wx, sum_v (float64); vmax, vmin (float64); argmax, argmin (int64 flat indices, the lowest among
	equals).  A label without pixels has count 0, the box (ny, -1, nx, -1), NaN extremes and -1 for their positions."""
	fields = ("count", "ymin", "ymax", "xmin", "xmax", "sum_w", "sum_wy", "sum_wx", "sum_v", "vmax", "vmin", "argmax", "argmin")
	def __init__(self, shape, nlabel, **arrays):
		self.shape, self.nlabel = tuple(shape), int(nlabel)
		for k in self.fields: setattr(self, k, arrays[k])
	def center_of_mass(self):
		"""[nlabel, {y,x}]: sum_w{y,x} / sum_w"""
		stack = A.torch().stack if A.is_tensor(self.sum_w) else np.stack
		return stack([self.sum_wy/self.sum_w, self.sum_wx/self.sum_w], -1)

def _check_size(shape):
	if len(shape) != 2: raise ValueError("labels works on 2-D maps [ny, nx]")
	if int(shape[0])*int(shape[1]) >= MAX_PIX:
		raise _lib.PxsError(-1, "label: the map must have fewer than 2^31 pixels, got %d x %d" % (int(shape[0]), int(shape[1])))

def _mask8(x, device):
	"""a mask of any dtype as the uint8 array the kernel reads: non-zero is set"""
	return A.put(x if A.np_dtype(x) == np.dtype(np.uint8) else (x != 0), np.uint8, device)

def _plain(x):
	x = A.unwrap(x)
	return x if x is None or A.is_tensor(x) else np.asarray(x)

def label(mask, connectivity=1, wrap=False):
	"""The connected components of the non-zero pixels of mask [ny, nx] (any dtype): (labels, n), labels int32 with 0 for the background and
	1 .. n for the components in ascending order of their lowest flat pixel index, as scipy.ndimage.label numbers them.  connectivity 1:
	4-neighbours (scipy's default structure), 2: 8-neighbours.  wrap: column nx-1 is a neighbour of column 0, for maps that go round the
	sky.  A pure function of the mask, bit for bit.  ny*nx must be below 2^31."""
	if connectivity not in (1, 2): raise ValueError("connectivity must be 1 or 2")
	arr = _plain(mask)
	_check_size(arr.shape)
	device = A.device_of(arr)
	ny, nx = int(arr.shape[0]), int(arr.shape[1])
	if ny == 0 or nx == 0: raise ValueError("label needs a map with pixels")
	d = _mask8(arr, device)
	out = A.empty((ny, nx), np.int32, device=device)
	n = ctypes.c_int64(0)
	_lib.check(_lib.load().pxm_label(ny, nx, A.ptr(d), int(connectivity), int(bool(wrap)), A.ptr(out), ctypes.byref(n), A.device_index(), A.current_stream()))
	if device is None: out = A.host(out)
	if hasattr(mask, "wcs"): out = enmap.dmap(out, mask.wcs) if device is not None else enmap.ndmap(out, mask.wcs)
	return out, int(n.value)

def _real(x, shape, device, name):
	if x is None: return None, 0
	x = _plain(x)
	if tuple(x.shape) != tuple(shape): raise ValueError("%s must have the shape of the labels" % name)
	dt = A.np_dtype(x) if A.np_dtype(x) in (np.dtype(np.float32), np.dtype(np.float64)) else np.dtype(np.float64)
	return A.put(x, dt, device), A.DT[dt]

def stats(labels, values=None, weights=None, nlabel=None):
	"""Every per-label reduction over labels [ny, nx] (integers 0 .. nlabel, 0 is skipped) in one pass: a LabelStats.  values, weights:
	float32 or float64 maps of that shape (other dtypes are converted to float64); without weights w = 1, without values sum_v is 0 and the
	extremes are empty.  nlabel: the number of labels (default: the largest label of the map, which costs a reduction); a label above it
	is an error.  Everything but the four sums is independent of the order of execution."""
	lab = _plain(labels)
	if lab.ndim != 2: raise ValueError("stats needs a 2-D label map")
	device = A.device_of(lab, values, weights)
	ny, nx = int(lab.shape[0]), int(lab.shape[1])
	d = A.put(lab, np.int32, device)
	if nlabel is None: nlabel = max(int(d.max()), 0) if ny*nx > 0 else 0
	nlabel = int(nlabel)
	if nlabel < 0: raise ValueError("nlabel must not be negative")
	dv, vdt = _real(values, (ny, nx), device, "values")
	dw, wdt = _real(weights, (ny, nx), device, "weights")
	count = A.empty((nlabel,), np.int64, device=device); box = A.empty((4, nlabel), np.int32, device=device)
	sums = A.empty((4, nlabel), np.float64, device=device)
	vmax, vmin = A.empty((nlabel,), np.float64, device=device), A.empty((nlabel,), np.float64, device=device)
	amax, amin = A.empty((nlabel,), np.int64, device=device), A.empty((nlabel,), np.int64, device=device)
	if ny*nx > 0:
		_lib.check(_lib.load().pxm_label_stats(ny, nx, A.ptr(d), nlabel, A.ptr(dv), vdt, A.ptr(dw), wdt, A.ptr(count), A.ptr(box), A.ptr(sums),
			A.ptr(vmax), A.ptr(vmin), A.ptr(amax), A.ptr(amin), A.device_index(), A.current_stream()))
	out = lambda a: a if device is not None else A.host(a)
	return LabelStats((ny, nx), nlabel, count=out(count), ymin=out(box[0]), ymax=out(box[1]), xmin=out(box[2]), xmax=out(box[3]),
		sum_w=out(sums[0]), sum_wy=out(sums[1]), sum_wx=out(sums[2]), sum_v=out(sums[3]), vmax=out(vmax), vmin=out(vmin), argmax=out(amax), argmin=out(amin))

# ---- scipy.ndimage's readers ----------------------------------------------------------------------------------------------------------
def _table(input, labels, index, weighted):
	"""the table the readers of `input` look at, and the rows `index` names: labels=None is the whole map as label 1, index=None the
	non-zero labels together as label 1 (scipy's rules)"""
	inp = _plain(input)
	if labels is None:
		lab = A.zeros(tuple(inp.shape), np.int32, like=inp) + 1; index = 1
	else:
		lab = _plain(labels)
		if index is None: lab = A.astype(lab != 0, np.int32); index = 1
	nlabel = None if index is None else max(int(np.max(np.asarray(index), initial=0)), 0)
	if nlabel is not None and lab.shape[0]*lab.shape[1] > 0: nlabel = max(nlabel, int(lab.max()))
	st = stats(lab, values=None if weighted else inp, weights=inp if weighted else None, nlabel=nlabel)
	return st, index

def _pick(st, arr, index, empty):
	"""arr[index-1], `empty` where index is not a label of the table; a scalar index gives a scalar (0-d) result"""
	idx = np.asarray(index, np.int64)
	ok = (idx >= 1) & (idx <= st.nlabel)
	sel = np.where(ok, idx-1, 0)
	if st.nlabel == 0:
		res = np.full(idx.shape+tuple(arr.shape[1:]), empty, A.np_dtype(arr))
		return A.torch().as_tensor(res, device=arr.device) if A.is_tensor(arr) else res
	if A.is_tensor(arr):
		t = A.torch()
		res = arr[t.as_tensor(sel.reshape(-1), device=arr.device)].reshape(idx.shape+tuple(arr.shape[1:]))
		if not ok.all(): res = res.clone(); res[t.as_tensor(~ok, device=arr.device)] = empty
		return res
	res = np.array(arr[sel])
	if not ok.all(): res[~ok] = empty
	return res

def center_of_mass(input, labels=None, index=None):
	"""The centre of mass (y, x), weighted by input, of the pixels of each label of index (scipy.ndimage.center_of_mass): [2] for a scalar
	index, [nindex, 2] for a list."""
	st, index = _table(input, labels, index, True)
	return _pick(st, st.center_of_mass(), index, np.nan)

def sum_labels(input, labels=None, index=None):
	"""The sum of input over each label of index (scipy.ndimage.sum_labels)"""
	st, index = _table(input, labels, index, False)
	return _pick(st, st.sum_v, index, 0.0)

def maximum(input, labels=None, index=None):
	"""The maximum of input over each label of index (scipy.ndimage.maximum); NaN for a label without pixels"""
	st, index = _table(input, labels, index, False)
	return _pick(st, st.vmax, index, np.nan)

def minimum(input, labels=None, index=None):
	"""The minimum of input over each label of index (scipy.ndimage.minimum); NaN for a label without pixels"""
	st, index = _table(input, labels, index, False)
	return _pick(st, st.vmin, index, np.nan)

def _position(st, arg, index):
	flat = _pick(st, arg, index, -1)
	stack = A.torch().stack if A.is_tensor(flat) else np.stack
	nx = max(st.shape[1], 1)
	return stack([flat//nx, flat % nx], -1)

def maximum_position(input, labels=None, index=None):
	"""The first pixel (y, x), in raster order, that holds the maximum of each label of index (scipy.ndimage.maximum_position): [2] or
	[nindex, 2], int64; a label without pixels has no position (its flat index is -1)"""
	st, index = _table(input, labels, index, False)
	return _position(st, st.argmax, index)

def minimum_position(input, labels=None, index=None):
	"""The first pixel (y, x) that holds the minimum of each label of index (scipy.ndimage.minimum_position)"""
	st, index = _table(input, labels, index, False)
	return _position(st, st.argmin, index)

def find_objects(labels, max_label=0):
	"""The bounding box of each label 1 .. max_label (0: the largest label) as a tuple of slices, None for a label without pixels
	(scipy.ndimage.find_objects).  The boxes come to the host: they are four numbers per label."""
	st = stats(labels, nlabel=None if max_label < 1 else max_label)
	y0, y1, x0, x1, cnt = (A.host(a) for a in (st.ymin, st.ymax, st.xmin, st.xmax, st.count))
	return [(slice(int(y0[i]), int(y1[i])+1, None), slice(int(x0[i]), int(x1[i])+1, None)) if cnt[i] > 0 else None for i in range(st.nlabel)]
