"""The stand-in rank of tests/test_rank_group.py, host code only:

    python -m tests.rank_selftest_worker REGION RANK WORLD OUT_DIR ROUNDS BAD_RANK HOW [MARKER]

Every rank maps REGION and runs gbp_comm_region_selftest for ROUNDS rounds (gather, barrier); it exits with 4 where that fails, which is
how a rank leaves an aborted region.  Rank BAD_RANK first misbehaves as HOW says: `noisy` writes 1 MB to stderr, `exit3` writes a line
to stderr and exits with 3, `sleep` never arrives.  MARKER, if given, is a file every rank creates as soon as it runs."""
import os
import sys
import time

os.environ["GBP_NO_TORCH"] = "1"      # host calls only: the library is loaded without bringing torch's HIP runtime in first

from tests.rank_group import mapped_region, write_rank


def main(argv):
    region_path, rank, world, out_dir, rounds, bad_rank, how = argv[0], int(argv[1]), int(argv[2]), argv[3], int(argv[4]), int(argv[5]), argv[6]
    if len(argv) > 7:
        open(argv[7], "w").close()
    if rank == bad_rank:
        if how == "noisy":
            sys.stderr.write((("rank %d is noisy" % rank).ljust(63) + "\n") * 16384)
            sys.stderr.flush()
        elif how == "exit3":
            sys.stderr.write("rank %d gives up before its first barrier\n" % rank)
            return 3
        elif how == "sleep":
            time.sleep(600)
    from gbp_poplar_amd._lib import load
    lib = load()
    with mapped_region(region_path) as address:
        if lib.gbp_comm_region_selftest(address, rank, world, rounds) != 0:
            sys.stderr.write("rank %d: %s\n" % (rank, lib.gbp_last_error(None).decode()))
            return 4
    write_rank(out_dir, rank, {}, {"rank": rank, "rounds": rounds})
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
