"""Child of tests/test_detect_gpu.py's kernel-trace test, run under rocprofv3 in a process of its own: the sweep of tests/detect_sweep.py, which
launches every instantiation of libfeather_detect.so once and compares with the restatement as it goes."""
import detect_sweep as SW
import side_contract


def main():
    lib = side_contract.library("detect")
    seen = []
    SW.sweep(lib, seen.append)
    print(f"{len(seen)} launches of {len(set(seen))} routes")
    print("child ok")


if __name__ == "__main__":
    main()
