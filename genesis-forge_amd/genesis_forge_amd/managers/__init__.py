from .base import BaseManager
from .reward_manager import RewardManager
from .termination_manager import TerminationManager
from .action import BaseActionManager, DelayedPositionActionManager, PositionActionManager, PositionWithinLimitsActionManager
from .command import CommandManager, VelocityCommandManager
from .gait_command import GaitCommandManager
from .contact import ContactManager
from .terrain_manager import TerrainManager
from .height_scanner import HeightScanner
from .ray_caster import RayCaster
from .terrain_curriculum import TerrainCurriculum
from .push import PushDisturbance
from .action_delay import ActuatorDelay
from .entity_manager import EntityManager
from .observation_manager import ObservationManager
from .config import MdpFnClass, ResetMdpFnClass

__all__ = [
    "BaseManager", "RewardManager", "TerminationManager", "CommandManager", "VelocityCommandManager", "GaitCommandManager",
    "BaseActionManager", "PositionActionManager", "PositionWithinLimitsActionManager", "DelayedPositionActionManager", "ActuatorDelay", "ContactManager",
    "TerrainManager", "HeightScanner", "RayCaster", "TerrainCurriculum", "PushDisturbance", "EntityManager", "ObservationManager", "MdpFnClass", "ResetMdpFnClass",
]
