"""Worker for tests/test_fit_host.py (one process per rank, gloo backend, CPU tensors): each rank holds the statistics of its
part of the rows; `dist.merge_statistics` leaves every rank with the rank-order merge."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    out_dir = sys.argv[1]
    import torch
    import test_fit_host as T
    from lsm_speech_classifier_amd import dist as lsm_dist
    rank, _, world = lsm_dist.init("gloo")
    _, parts = T._halves()
    mine = parts[rank]
    before = mine.packed_gram().tobytes()
    merged = lsm_dist.merge_statistics(mine)
    assert merged is not mine and mine.packed_gram().tobytes() == before          # the rank's own statistics are left alone
    merged.save(os.path.join(out_dir, f"rank{rank}.npz"))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
