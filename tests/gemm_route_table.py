"""The route table of the update GEMM: which options (gpmi_dev_set_option) and shapes reach which kernel -- TEST
INFRASTRUCTURE shared by tests/test_gemm_routes_gpu.py, which runs every (route, case) on the GPU against the contract
of gemm_contract.py, and tests/test_gemm_route_cpu.py, which asks the library's one route function (csrc/gpmi_route.h:
gemm_route) for the kernel of every (route, case) and asserts the name written here."""
from gemm_contract import Case

DEFAULTS = dict(gemm_dma=1, gemm_small_tiles=1, gemm_small_dma=1, gemm_persist=1, gemm_ticket=0, gemm_dma_waves=8,
                gemm_tall=1, tall_min_tiles=12288)


def _lowers(M, N, K):
    # diag_off: on the diagonal, panel_rec's -64, above it, well below it, everything live, nothing live
    return [Case(M, N, K, lower=1, diag_off=o) for o in (0, -64, 128, -384, N, -M)]


# fewer than 128 tiles of 128 x 128
SMALL = [Case(640, 640, 16), Case(640, 640, 48), Case(640, 640, 256), Case(640, 640, 1040),
         Case(384, 1088, 48), Case(1280, 704, 48),
         *_lowers(1024, 1024, 48), Case(640, 640, 1040, lower=1, diag_off=-64), Case(1280, 768, 48, lower=1)]
# row maps: reaches off the 128 grid, an empty band, bands of three tiles, a partial last band
SMALL_MAPS = [Case(640, 768, 48, reach=(300, 0, 768, 129, 700)),
              Case(640, 768, 48, reach=(300, 0, 768, 129, 700), host_map=False),
              Case(896, 640, 32, reach=(200, 640, 520), rbr=384),
              Case(896, 640, 1040, reach=(200, 640, 520), rbr=384, host_map=False)]
# N % 128 == 64
ODD64 = [Case(640, 704, 48), Case(384, 1088, 1040), Case(640, 704, 16), *_lowers(1024, 1088, 48),
         Case(640, 832, 48, reach=(100, 832, 0, 577, 64)), Case(896, 832, 48, reach=(300, 700, 832), rbr=384, host_map=False),
         Case(1536, 1600, 48)]
# 128 tiles and more (an odd number of tile rows splits the tall form's pairs)
BIG = [Case(1664, 1664, 32), Case(1664, 1664, 48), Case(1664, 1664, 256), Case(1664, 1664, 1040), Case(1664, 1664, 16),
       Case(1408, 1920, 48), Case(1920, 1152, 256),
       *_lowers(1664, 1664, 48), Case(1664, 1664, 1040, lower=1, diag_off=-64), Case(1920, 1152, 48, lower=1)]
BIG_MAPS = [Case(1920, 1920, 48, reach=tuple(min(1920, 300 + 131 * q) for q in range(14)) + (0,)),
            Case(1920, 1920, 48, reach=tuple(min(1920, 300 + 131 * q) for q in range(14)) + (0,), host_map=False),
            Case(1920, 1920, 272, reach=(129, 1920, 700, 1000, 1), rbr=384),
            Case(1920, 1920, 48, reach=(700, 1920, 1300, 1025), rbr=512),
            Case(1920, 1920, 48, reach=(700, 1920, 1300, 1025), rbr=512, host_map=False)]
BLOCKS = [Case(1536, 1920, 48, brows=256),
          Case(1536, 1920, 48, reach=tuple(min(1920, 100 + 250 * q) for q in range(12)), brows=256),
          Case(1536, 1920, 1040, reach=(1920, 640, 1500, 129), rbr=384, brows=384)]
# at least two rounds of 256 blocks with K >= 256 (persistent), at least one round (ticket)
# (a staircase with its host copy launches only its live supertiles: 30 bands, so that they still make two rounds)
STAIRS = tuple(2944 - 29 * q for q in range(30))
PERSIST = [Case(2944, 2944, 256), Case(2944, 2944, 272),
           Case(3840, 2944, 256, reach=STAIRS),
           Case(3840, 2944, 256, reach=STAIRS, host_map=False),
           Case(3840, 2944, 256, reach=STAIRS, brows=256)]
TICKET = [Case(2304, 2304, 48), Case(2304, 2304, 1040),
          Case(2304, 2304, 48, reach=tuple(2304 - 37 * q for q in range(18))),
          Case(2304, 2304, 48, reach=tuple(2304 - 37 * q for q in range(18)), host_map=False),
          Case(2304, 2304, 48, reach=tuple(2304 - 37 * q for q in range(18)), brows=256)]

# name: (options, under gpmi_dev_set_concurrent(1), kernel, cases)
ROUTES = {
    "small_dma8": ({}, False, "gemm_nt_small_kernel<8>", SMALL),
    "small_dma3": ({}, True, "gemm_nt_small_kernel<3>", SMALL),
    "reg64": ({"gemm_small_dma": 0}, False, "gemm_nt_kernel<2, 2, false>", SMALL + SMALL_MAPS),
    "reg128": ({"gemm_dma": 0, "gemm_small_tiles": 0}, False, "gemm_nt_kernel<4, 4, false>",
               [c for c in SMALL if c.N % 128 == 0] + SMALL_MAPS + [Case(1664, 1664, 1040, lower=1, diag_off=-64)]),
    "reg128x64": ({"gemm_small_tiles": 0}, False, "gemm_nt_kernel<4, 2, false>", ODD64),
    "dma8": ({"gemm_persist": 0, "gemm_tall": 0}, False, "gemm_nt_dma_kernel<2, false>", BIG + BIG_MAPS + BLOCKS),
    "dma4": ({"gemm_persist": 0, "gemm_tall": 0, "gemm_dma_waves": 4}, False, "gemm_nt_dma_kernel<4, false>",
             BIG + BIG_MAPS + BLOCKS),
    "tall": ({"gemm_persist": 0, "gemm_tall": 1, "tall_min_tiles": 0}, False, "gemm_nt_dma_tall_kernel<false>",
             BIG + BIG_MAPS + BLOCKS),
    "persist": ({}, False, "gemm_nt_dma_persist_kernel", PERSIST),
    "ticket": ({"gemm_ticket": 2}, False, "gemm_nt_dma_ticket_kernel", TICKET),
}

# (route, case) that do not reach the route's kernel, with the kernel they do reach.  K = 16 is one K step: the LDS-DMA
# family keeps two in flight and takes K >= 32, so under the options of dma8 / dma4 / tall the launch runs on the
# first-generation 128 x 128 kernel.  The case stays in the GPU test (the contract holds on whatever kernel runs); the
# three routes keep K = 32 as their shortest K.
REACHES = {(name, Case(1664, 1664, 16)): "gemm_nt_kernel<4, 4, false>" for name in ("dma8", "dma4", "tall")}


def kernel(name, case):
    """the kernel (route, case) reaches on a device with a counter pool for the resident forms"""
    return REACHES.get((name, case), ROUTES[name][2])


# what the resident routes reach on a device without a counter pool: one workgroup per tile, the same bits
NO_POOL = {"persist": "gemm_nt_dma_kernel<2, false>", "ticket": "gemm_nt_dma_kernel<2, false>"}


# full-mantissa operands on every route: a plain launch, lower mode on an odd offset, a row map
BOUND = {
    "small_dma8": [Case(640, 640, 1040), Case(1024, 1024, 48, lower=1, diag_off=-64)],
    "small_dma3": [Case(640, 640, 1040), Case(1024, 1024, 48, lower=1, diag_off=-64)],
    "reg64": [Case(640, 640, 1040), Case(1024, 1024, 48, lower=1, diag_off=-64), SMALL_MAPS[2]],
    "reg128": [Case(640, 640, 1040), Case(1024, 1024, 48, lower=1, diag_off=-64), SMALL_MAPS[2]],
    "reg128x64": [Case(384, 1088, 1040), Case(1024, 1088, 48, lower=1, diag_off=-64), ODD64[-2]],
    "dma8": [Case(1664, 1664, 1040), Case(1664, 1664, 48, lower=1, diag_off=-64), BIG_MAPS[2], BLOCKS[2]],
    "dma4": [Case(1664, 1664, 1040), Case(1664, 1664, 48, lower=1, diag_off=-64), BIG_MAPS[2], BLOCKS[2]],
    "tall": [Case(1664, 1664, 1040), Case(1664, 1664, 48, lower=1, diag_off=-64), BIG_MAPS[2], BLOCKS[2]],
    "persist": [PERSIST[1], PERSIST[2]],
    "ticket": [TICKET[1], TICKET[2]],
}
