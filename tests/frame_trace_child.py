"""Child of tests/test_frame_gpu.py's kernel-trace test, run under rocprofv3 in a process of its own: the sweep of tests/frame_sweep.py, which
launches every instantiation of libfeather_frame.so once and compares with the restatement as it goes.  It prints the routes
fhip_frame_route named, in launch order, for the parent to hold against the trace."""
import frame_sweep as SW
import side_contract


def main():
    lib = side_contract.library("frame")
    seen = []
    SW.sweep(lib, seen.append)
    for name in seen:
        print("route " + name)
    print(f"{len(seen)} launches of {len(set(seen))} routes")
    print("child ok")


if __name__ == "__main__":
    main()
