"""bm2f_amd.label_planes: the one rule by which an integer label map reaches the label kernels, written out as a
table, and ``_native.upload_tables`` on a CPU device.  The expected dtypes are the rule's own statement: a dtype the
kernels read comes back as the same object, any other integer dtype becomes int32 in the same container, float and
bool are refused."""
import numpy as np
import pytest
import torch

from bm2f_amd import PanopticGroundTruth, _native
from bm2f_amd.label_planes import LABEL_DTYPES, WIDE_DTYPE, as_label_maps, as_label_plane, np_dtype, same_dtype
from bm2f_amd.panoptic_eval import panoptic_counts

# dtype name -> what as_label_plane answers without / with ``wide``: "same" (the object itself), "int32", or the key
# words of the ValueError
RULE = {
    "bool": ("integer labels", "integer labels"),
    "float32": ("integer labels", "integer labels"),
    "int8": ("int32", "int32"),
    "uint8": ("same", "same"),
    "int16": ("same", "same"),
    "int32": ("same", "same"),
    "int64": ("int32", "same"),
    "uint16": ("int32", "int32"),
    "uint32": ("int32", "int32"),
}
TORCH_NAMES = ["bool", "float32", "int8", "uint8", "int16", "int32", "int64"]


def _make(container, name):
    a = np.arange(12).reshape(3, 4).astype(name)
    return a if container == "numpy" else torch.from_numpy(a)


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("container,name", [("numpy", n) for n in RULE] + [("torch", n) for n in TORCH_NAMES])
def test_as_label_plane_rule(container, name, wide):
    x = _make(container, name)
    want = RULE[name][wide]
    if want == "integer labels":
        with pytest.raises(ValueError, match=f"the map must hold integer labels, got .*{name}"):
            as_label_plane(x, "the map", wide=wide)
        return
    got = as_label_plane(x, "the map", wide=wide)
    assert torch.is_tensor(got) == (container == "torch") and isinstance(got, np.ndarray) == (container == "numpy")
    if want == "same":
        assert got is x
    else:
        assert got is not x and np_dtype(got.dtype) == np.int32
        assert np.array_equal(np.asarray(got), np.arange(12).reshape(3, 4))


def test_as_label_plane_range_check_of_arrays():
    for value in (2 ** 31, 2 ** 32 - 1):
        with pytest.raises(ValueError, match="the map holds labels beyond int32"):
            as_label_plane(np.array([[0, value]], dtype=np.uint32), "the map")
    with pytest.raises(ValueError, match="beyond int32"):
        as_label_plane(np.array([[-2 ** 31 - 1]], dtype=np.int64), "the map")
    got = as_label_plane(np.array([[-2 ** 31, 2 ** 31 - 1]], dtype=np.int64), "the map")     # the ends of the range fit
    assert got.dtype == np.int32 and got.tolist() == [[-2 ** 31, 2 ** 31 - 1]]
    wide = np.array([[2 ** 40]], dtype=np.int64)
    assert as_label_plane(wide, "the map", wide=True) is wide                                # read as it is: no check
    assert as_label_plane(np.zeros((0, 3), np.uint32), "the map").dtype == np.int32          # nothing to check
    assert as_label_plane([[1, 2], [3, 4]], "the map", wide=True).dtype == np.int64          # a list is an array


def test_dtype_table_and_names():
    assert list(LABEL_DTYPES) == [torch.uint8, torch.int16, torch.int32] and WIDE_DTYPE == torch.int64
    for dtype, (nbytes, lo, hi) in LABEL_DTYPES.items():
        info = torch.iinfo(dtype)
        assert (nbytes, lo, hi) == (info.bits // 8, info.min, info.max)
        assert np_dtype(dtype) == np_dtype(np_dtype(dtype)) == np.dtype(str(dtype)[6:])
    assert np_dtype(torch.int64) == np.int64 and np_dtype(np.uint16) == np.uint16
    assert np_dtype(torch.bfloat16) == np.dtype(object)                                      # numpy has no such name


def test_same_dtype():
    a, b, c = np.zeros((2, 2), np.uint8), torch.ones((3, 1), dtype=torch.int16), np.full((1, 4), 70000, np.int32)
    got = same_dtype([a, b, c])
    assert [np_dtype(p.dtype) for p in got] == [np.int32] * 3
    assert isinstance(got[0], np.ndarray) and torch.is_tensor(got[1]) and got[2] is c
    assert not got[0].any() and got[1].tolist() == [[1], [1], [1]]
    got = same_dtype([b, a])
    assert got[0] is b and got[1].dtype == np.int16
    got = same_dtype([np.zeros(3, np.int32), np.zeros(3, np.int64)])                          # the wide side
    assert [p.dtype for p in got] == [np.int64, np.int64]
    equal = [a, torch.zeros((5, 5), dtype=torch.uint8)]
    assert same_dtype(equal) is equal
    empty = []
    assert same_dtype(empty) is empty


def test_as_label_maps():
    from bm2f_amd import label_targets
    assert label_targets.as_label_maps is as_label_maps
    wide = torch.arange(6, dtype=torch.int64).reshape(2, 3)
    got, = as_label_maps([wide])
    assert got.dtype == torch.int32 and got.is_contiguous() and torch.equal(got, wide.to(torch.int32))
    mixed = as_label_maps([torch.zeros((2, 2), dtype=torch.uint8), np.ones((3, 2), np.int16),
                           torch.full((1, 1), -3, dtype=torch.int8)])
    assert [m.dtype for m in mixed] == [torch.int32] * 3 and mixed[2].item() == -3 and mixed[1].tolist() == [[1, 1]] * 3
    strided = torch.arange(24, dtype=torch.uint8).reshape(4, 6)[:, ::2]
    uniform = as_label_maps([strided, torch.zeros((2, 2), dtype=torch.uint8)])
    assert [m.dtype for m in uniform] == [torch.uint8] * 2 and all(m.is_contiguous() for m in uniform)
    assert torch.equal(uniform[0], strided)
    for bad in (torch.zeros((2, 2)), torch.zeros((2, 2), dtype=torch.bool), torch.zeros(4, dtype=torch.int32)):
        with pytest.raises(ValueError, match=r"pan_seg of image 0 must be an \(H, W\) integer tensor"):
            as_label_maps([bad], "pan_seg")


def _panoptic_case():
    rng = np.random.RandomState(3)
    gt_ids = np.array([0, 5, 70000, 2 ** 24 - 1])
    id_map = gt_ids[rng.randint(0, 4, size=(11, 19))].astype(np.int32)
    js = {"categories": [{"id": 1, "isthing": 1}, {"id": 2, "isthing": 0}],
          "annotations": [{"image_id": 7, "file_name": None,
                           "segments_info": [{"id": 5, "category_id": 1}, {"id": 70000, "category_id": 2},
                                             {"id": 2 ** 24 - 1, "category_id": 1, "iscrowd": 1}]}]}
    pred = rng.randint(0, 4, size=(11, 19)).astype(np.int32)
    info = [{"id": k, "category_id": 1 + k % 2} for k in (1, 2, 3)]
    return PanopticGroundTruth(js, {7: id_map}), id_map, pred, info


def test_panoptic_counts_numpy_prediction_in_an_unlisted_dtype():
    """A numpy prediction in uint16 (int8, uint32, uint64 alike) is counted as its int32 copy; such an array holding a
    value from 2^31 on is refused for its range before anything is counted."""
    gt, id_map, pred, info = _panoptic_case()
    (want, _, want_rows), = panoptic_counts(gt, [(7, pred, info)])
    assert want.sum() == pred.size and want.shape == (5, 4)
    for dtype in (np.uint16, np.int8, np.uint32, np.uint64, np.int64):
        (got, _, rows), = panoptic_counts(gt, [(7, pred.astype(dtype), info)])
        assert np.array_equal(got, want) and np.array_equal(rows, want_rows), dtype
    (got, _, _), = panoptic_counts(gt, [(7, torch.from_numpy(pred.astype(np.int8)), info)], device="cpu")
    assert np.array_equal(got, want)
    (got, _, _), = panoptic_counts(gt, [(7, pred.astype(np.uint16), info)], device="cpu")    # uploaded as a tensor
    assert np.array_equal(got, want)
    beyond = pred.astype(np.uint32)
    beyond[0, 0] = 2 ** 31
    with pytest.raises(ValueError, match="panoptic_seg holds labels beyond int32"):
        panoptic_counts(gt, [(7, beyond, info)])
    with pytest.raises(ValueError, match="panoptic_seg must hold integer labels"):
        panoptic_counts(gt, [(7, pred.astype(np.float32), info)])
    listed = pred.astype(np.int64)
    listed[0, 0] = 2 ** 31                                   # int64 is read as it is: the panopticapi-worded error
    with pytest.raises(KeyError, match="segment with ID 2147483648"):
        panoptic_counts(gt, [(7, listed, info)])


def test_panoptic_ground_truth_id_map_is_int32():
    gt, id_map, _, _ = _panoptic_case()
    assert gt.id_map(7).dtype == np.int32 and np.array_equal(gt.id_map(7), id_map)
    gt.id_maps[7] = torch.from_numpy(id_map.astype(np.int64))
    assert gt.id_map(7).dtype == torch.int32 and np.array_equal(gt.id_map(7).numpy(), id_map)
    gt.id_maps[7] = id_map.astype(np.uint8)
    assert gt.id_map(7).dtype == np.int32                     # always int32, whatever the kernels would read
    for bad in (id_map.astype(np.float64), torch.zeros((11, 19), dtype=torch.bool)):
        gt.id_maps[7] = bad
        with pytest.raises(ValueError, match="image 7: the id map must hold integer"):
            gt.id_map(7)


@pytest.mark.parametrize("lengths", [(3, 0, 5, 1), (0,), (1, 1, 1), (0, 0), (4, 7)])
def test_upload_tables_round_trip(lengths):
    rng = np.random.RandomState(sum(lengths))
    tables = {}
    for k, n in enumerate(lengths):
        tables[f"i{k}"] = rng.randint(-2 ** 31, 2 ** 31, size=n, dtype=np.int64).astype(np.int32)
        tables[f"l{k}"] = rng.randint(-2 ** 62, 2 ** 62, size=n, dtype=np.int64)
    tables["matrix"] = rng.randint(0, 9, size=(3, 3)).astype(np.int32)                       # flattened, odd length
    dev = _native.upload_tables(tables, torch.device("cpu"))
    assert set(dev) == set(tables) | {"_buffer"}
    buf = dev["_buffer"]
    assert buf.dtype == torch.int32 and buf.dim() == 1 and buf.numel() % 2 == 0
    at = 0
    for name, arr in tables.items():
        t = dev[name]
        assert t.dtype == (torch.int64 if arr.dtype == np.int64 else torch.int32), name
        assert np.array_equal(t.numpy(), arr.reshape(-1)), name
        assert at % 2 == 0                                             # in order, each on an 8-byte boundary
        if arr.size:
            assert t.data_ptr() - buf.data_ptr() == 4 * at and t.data_ptr() % 8 == 0, name
        at += arr.size * (2 if arr.dtype == np.int64 else 1)
        at += at % 2
    assert buf.numel() == max(at, 2)


def test_upload_tables_of_nothing():
    dev = _native.upload_tables({}, torch.device("cpu"))
    assert list(dev) == ["_buffer"] and dev["_buffer"].numel() == 2
    dev = _native.upload_tables({"a": np.zeros(0, np.int64), "b": np.zeros(0, np.int32)}, torch.device("cpu"))
    assert dev["a"].dtype == torch.int64 and dev["a"].numel() == 0 and dev["b"].numel() == 0
    assert dev["_buffer"].numel() == 2
