"""Model constants consumed by the hot path.

Mirrors the model section of the reference's ``params.py:24-32`` (``T, M_VGGISH,
M_VGGISH_JB, H, DR, K, S_VGGISH_SHAPE``) and the class labels (``params.py:15-16``: UrbanSound8K's ten
classes in classID order, used by ``train.test_model``'s report). The dataset paths and the
ResNet constants are ``S_RESNET_SHAPE`` / ``M_RESNET`` (params.py:23-27). ``model.py`` binds these at import time exactly as the reference's
``from params import *`` does (``model.py:9``), so they are compile-time
constants of the model and of the HIP kernels instantiated for it.
"""

S_VGGISH_SHAPE = (96, 64)     # one VGGish example: 96 STFT frames x 64 mel bands
T = 10                        # examples (0.96 s clips) per bag
M_VGGISH = 128                # VGGish embedding width
M_VGGISH_JB = 512 * 6 * 4     # flattened conv bottleneck width (just_bottlenecks=True)
S_RESNET_SHAPE = (224, 224)   # one ResNet-50 input image (params.py:23 of the reference)
M_RESNET = 2048               # ResNet-50 bottleneck width after the global average pool
H = 600                       # hidden width of the embedded mappings
DR = 0.4                      # dropout rate inside the embedded mappings
K = 10                        # classes
TARGET_NAMES = ["air_conditioner", "car_horn", "children_playing", "dog_bark", "drilling", "engine_idling", "gun_shot",
                "jackhammer", "siren", "street_music"]

BATCH_SIZE = 8
NUM_EPOCHS = 25
FEATURE_EXTRACT = True
LR = 0.001

# the ResNet branch's audio constants (params.py:8, :11-12 of the reference)
MAX_SECONDS = 4
SR_RESNET = 22_050
SAMPLES_NUM_RESNET = SR_RESNET * MAX_SECONDS
