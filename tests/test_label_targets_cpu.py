"""Label-map training targets on CPU tensors: the helpers against the restated reference mappers, the label
histogram against np.bincount, and the criterion / matcher against the dense equivalents of the same targets (the
plain-torch path: dense masks from the map, then the existing code).  No GPU needed.  The checks are in
label_target_cases.py, shared with the device tests."""
import pytest
import torch

import label_target_cases as cases

CPU = torch.device("cpu")
DTYPE_IDS = [str(d).replace("torch.", "") for d in cases.MAP_DTYPES]


@pytest.mark.parametrize("dtype", cases.MAP_DTYPES, ids=DTYPE_IDS)
def test_semantic_targets(dtype):
    cases.check_semantic_targets(CPU, dtype)


@pytest.mark.parametrize("dtype", cases.MAP_DTYPES, ids=DTYPE_IDS)
def test_panoptic_targets(dtype):
    cases.check_panoptic_targets(CPU, dtype)


@pytest.mark.parametrize("bins", [19, 150])
@pytest.mark.parametrize("dtype", cases.MAP_DTYPES[:3], ids=DTYPE_IDS[:3])
def test_label_histogram(dtype, bins):
    cases.check_histogram(CPU, dtype, bins)


def test_histogram_refuses_what_it_cannot_count():
    with pytest.raises(ValueError):
        cases.label_histogram_ragged([torch.zeros(2, 2, dtype=torch.int64)], 5)
    with pytest.raises(ValueError):
        cases.label_histogram_ragged([torch.zeros(2, 2, dtype=torch.uint8), torch.zeros(2, 2, dtype=torch.int32)], 5)
    counts, bad = cases.label_histogram_ragged([], 5)
    assert counts.shape == (0, 6) and bad.shape == (0,)


def test_criterion_label_maps_vs_dense():
    cases.check_criterion(CPU, bitwise=False)


def test_empty_cases_and_errors():
    cases.check_empty_and_errors(CPU, bitwise=False)
