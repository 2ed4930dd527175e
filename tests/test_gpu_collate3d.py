"""collate_cells3d_kernel and the three-level ragged kernels against the
nested-list reference of test_collate3d.py; the dataset's launch budget."""

import numpy as np
import pytest

import test_collate3d as C

pytestmark = pytest.mark.gpu


def to_device(sources):
    from spark_tfrecord_amd.engine import gpu as gpu_engine
    return [gpu_engine.batch_to_device(s) for s in sources]


@pytest.mark.parametrize("shape", C.SHAPES)
def test_padded3d_truncating(shape):
    C.padded_case("gpu", shape, True, to_device)


def test_padded3d_length_error():
    C.padded_case("gpu", C.SHAPES[1], False, to_device)


@pytest.mark.parametrize("short", [None, 0, 1, 2])
def test_ragged3d(short):
    C.ragged_case("gpu", short, to_device)


def test_dataset_gpu_equals_cpu(tmp_path):
    [(cpu, a), (gpu, b)], _ = C.dataset_case(tmp_path, ["cpu", "gpu"])
    assert len(a) == len(b) == 4
    for x, y in zip(a, b):
        assert set(x) == set(y) and all(t.is_cuda for t in y.values())
        for k in x:
            assert np.array_equal(x[k].numpy(), y[k].cpu().numpy()), k
    assert cpu.truncated_rows == gpu.truncated_rows > 0
    # dense 1 + packed 2, as before, and one for the Padded3D column
    assert gpu.last_stats == {"batches": 4, "launches": 16, "host_waits": 4}
