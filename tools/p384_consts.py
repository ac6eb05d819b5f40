"""Print the constant tables of minbft_amd/csrc/p384_fe.h from the curve's
parameters: p, N, b and G in 14 limbs of 28 bits, the Montgomery constants for
R = 2^392 and the word forms used by the range checks.

    python tools/p384_consts.py

The header's tables were pasted from this output; tests/test_p384_host.py
recomputes them and compares.
"""
P = 2**384 - 2**128 - 2**96 + 2**32 - 1
N = 0xffffffffffffffffffffffffffffffffffffffffffffffffc7634d81f4372ddf581a0db248b0a77aecec196accc52973
B = 0xb3312fa7e23ee7e4988e056be3f82d19181d9c6efe8141120314088f5013875ac656398d8a2ed19d2a85c8edd3ec2aef
GX = 0xaa87ca22be8b05378eb1c71ef320ad746e1d3b628ba79b9859f741e082542a385502f25dbf55296c3a545e3872760ab7
GY = 0x3617de4a96262c6f5d9e98bf9292dc29f8f41dbd289a147ce9da3113b5f0b8c00a60b1ce1d7e819d7a431d7c90ea0e5f
NL, LB = 14, 28
R = 1 << (NL * LB)


def limbs(v):
    """14 limbs of 28 bits; the top limb takes what is left (v < 2^396)."""
    out = [(v >> (LB * i)) & ((1 << LB) - 1) for i in range(NL - 1)]
    return out + [v >> (LB * (NL - 1))]


def words(v, n=12):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def table(name, vals, typ="uint32_t", n="NL384"):
    body = ", ".join("0x%08xu" % v for v in vals)
    return "P384_CONST %s %s[%s] = {%s};" % (typ, name, n, body)


def constants():
    """name -> list of words, everything the header holds."""
    return {
        "kP384": limbs(P), "kP384x32": limbs(32 * P),
        "kP384R": limbs(R % P), "kP384R2": limbs(R * R % P), "kP384B": limbs(B * R % P),
        "kP384Gx": limbs(GX * R % P), "kP384Gy": limbs(GY * R % P),
        "kN384": limbs(N), "kN384R2": limbs(R * R % N),
        "kN384INV": [(-pow(N, -1, 1 << LB)) % (1 << LB)],
        "kP384w": words(P), "kN384w": words(N), "kPmN384w": words(P - N),
        "kExpP384m2": words(P - 2)[::-1], "kExpN384m2": words(N - 2)[::-1],
    }


if __name__ == "__main__":
    for k, v in constants().items():
        if k == "kN384INV":
            print("constexpr uint32_t kN384INV = 0x%08xu;" % v[0])
        else:
            print(table(k, v, n="NL384" if len(v) == NL else "12"))
