"""The five model families the physics layer is built for, by the short names the tests and the rate tools use."""

FAMILIES = ("cube", "tshape", "go2flat", "go2rough", "footstand")
_GO2 = {"go2flat": "Go2JoystickFlatTerrain", "go2rough": "Go2JoystickRoughTerrain", "footstand": "Go2Footstand"}


def envdef(kind):
    """the env definition of a family (no batch, no device)"""
    from rsr_mjx_amd.envs import airbot, go2
    if kind in ("cube", "tshape"):
        return airbot.AirbotPlayBase() if kind == "cube" else airbot.AirbotTShape()
    return go2.load(_GO2[kind])
