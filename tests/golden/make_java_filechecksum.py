"""Write tests/golden/java_filechecksum.json: the five getFileChecksum results
the reference's Java SDK test asserts (sdk/java/src/test/java/io/juicefs/
JuiceFileSystemTest.java:492-531, testChecksum), taken as data.

Each case describes its file instead of holding it: a literal, or
{"zeros": n} for n zero bytes; `length` is getFileChecksum's second argument
(null: the whole file) and `block` the file system's block size in that test
(128 MiB).  `expect` is the checksum object the test compares with:
MD5MD5CRC32GzipFileChecksum is type "CRC32", MD5MD5CRC32CastagnoliFileChecksum
is "CRC32C", then (bytesPerCRC, crcPerBlock, MD5 hex).  These are the only
values the reference holds for the arithmetic of the CRC32C hot path.
Run: python tests/golden/make_java_filechecksum.py
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
BLOCK = 128 << 20

CASES = [
    ("empty", {"literal": ""}, None, ("CRC32", 0, 0, "70bc8f4b72a86921468bf8e8441dce51")),
    ("small", {"literal": "world\n"}, None, ("CRC32C", 512, 0, "a74dcf6d5ba98e50ae0182c9d5d886fe")),
    ("small_length5", {"literal": "world\n"}, 5, ("CRC32C", 512, 0, "05a157db1cc7549c82ec6f31f63fdb46")),
    ("medium", {"zeros": (128 << 20) - 1}, None, ("CRC32C", 512, 0, "1cf326bae8274fd824ec69ece3e4082f")),
    ("big", {"zeros": 150 * 1024 * 1000}, None, ("CRC32C", 512, 262144, "7d04ac8132ad64988f7ba4d819cbde62")),
]


def main():
    rows = [{"name": name, "content": content, "length": length, "block": BLOCK,
             "expect": {"type": e[0], "bytesPerCRC": e[1], "crcPerBlock": e[2], "md5": e[3]}}
            for name, content, length, e in CASES]
    with open(os.path.join(HERE, "java_filechecksum.json"), "w") as f:
        json.dump({"source": "sdk/java/src/test/java/io/juicefs/JuiceFileSystemTest.java:492-531", "cases": rows},
                  f, indent=1)
        f.write("\n")
    print("wrote %d cases" % len(rows))


if __name__ == "__main__":
    main()
