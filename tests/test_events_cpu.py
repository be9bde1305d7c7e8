"""``gnn_tracking_amd.events``: the offsets of the events of a collated batch from ``ptr`` / ``batch``, the two forms of
the sortedness check and the host validation of offsets.  Plain CPU tensors, no kernel."""

import numpy as np
import pytest
import torch

from gnn_tracking_amd import Data, events


def test_ptr_is_handed_through_and_one_event_is_none():
    ptr = torch.tensor([0, 3, 3, 5], dtype=torch.int32)
    got = events.event_ptr(ptr=ptr)
    assert got.dtype == torch.int64 and got.tolist() == [0, 3, 3, 5]
    same = torch.tensor([0, 2, 7])
    assert events.event_ptr(ptr=same) is same
    assert events.event_ptr(ptr=[0, 2, 7]).tolist() == [0, 2, 7]
    assert events.event_ptr(ptr=torch.tensor([0, 5])) is None and events.event_ptr(ptr=[0, 5]) is None
    assert events.event_ptr() is None and events.event_ptr(Data(x=torch.zeros(3, 2))) is None


def test_offsets_from_a_sorted_batch():
    got = events.event_ptr(batch=torch.tensor([0, 0, 2, 2, 2]))
    assert got.dtype == torch.int64 and got.tolist() == [0, 2, 2, 5], "an empty event in the middle stays an event"
    assert events.event_ptr(batch=torch.tensor([0, 0, 1], dtype=torch.int32)).tolist() == [0, 2, 3]
    assert events.event_ptr(batch=torch.zeros(4, dtype=torch.long)) is None
    assert events.event_ptr(batch=torch.zeros(0, dtype=torch.long)) is None
    # (offsets of a batch that lost rows to a mask are those of the rows that are left)
    batch = torch.tensor([0, 0, 1, 1, 1, 2])
    assert events.event_ptr(batch=batch[torch.tensor([True, False, True, True, False, True])]).tolist() == [0, 1, 3, 4]
    assert events.offsets_of(torch.zeros(4, dtype=torch.long)).tolist() == [0, 4]


def test_unsorted_batch_raising_and_deferred():
    bad = torch.tensor([0, 1, 0, 1])
    with pytest.raises(ValueError, match=r"^somebody: `batch` must be sorted \(PyG convention\)$"):
        events.event_ptr(batch=bad, who="somebody")
    with pytest.raises(ValueError, match="sorted"):
        events.event_ptr(Data(batch=bad), who="somebody")
    assert events.event_ptr(batch=bad, who=None).tolist() == [0, 2, 4]      # raises nothing: the flag is the caller's
    flag = events.unsorted(bad)
    assert torch.is_tensor(flag) and flag.dtype == torch.bool and flag.dim() == 0 and bool(flag)
    assert not bool(events.unsorted(torch.tensor([0, 0, 1, 3])))
    assert not bool(events.unsorted(torch.zeros(0, dtype=torch.long))) and not bool(events.unsorted(torch.tensor([4])))


@pytest.mark.parametrize("make", (torch.tensor, np.array, list), ids=("tensor", "numpy", "list"))
def test_host_validation(make):
    for ptr, n in (([1, 3, 5], 5), ([0, 3, 4], 5), ([0, 4, 3, 5], 5)):
        with pytest.raises(ValueError, match=r"^the caller: .*ascend") as err:
            events.event_sizes(make(ptr), n, "the caller")
        assert str(err.value) == "the caller: ptr must ascend from 0 to the number of hits"
    with pytest.raises(ValueError, match=r"^the caller: the offsets must ascend from 0 to the number of points$"):
        events.event_sizes(make([0, 3, 4]), 5, "the caller", "the offsets must ascend from 0 to the number of points")
    assert events.event_sizes(make([0, 3, 3, 5]), 5, "the caller") == [3, 0, 2]
    assert events.event_sizes(None, 5, "the caller") is None


def test_data_with_ptr_and_batch_uses_ptr():
    data = Data(ptr=torch.tensor([0, 1, 4]), batch=torch.tensor([1, 0, 0, 0]))     # (the batch is not even looked at)
    assert events.event_ptr(data).tolist() == [0, 1, 4]
    assert events.event_ptr(Data(batch=torch.tensor([0, 1, 1, 1]))).tolist() == [0, 1, 4]
    assert events.event_ptr(ptr=[0, 1, 4], batch=torch.tensor([1, 0, 0, 0])).tolist() == [0, 1, 4]
