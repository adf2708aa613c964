// `bf16 = true` in [network] (compute_dtype = PPO_DTYPE_BF16 through the facade), run in a fresh directory.
//   host_fused_bf16_test parse   (tests/test_fused_bf16_abi.py; no GPU needed): PPO_Discrete reads the key from PPOConfig.toml and prints it like the other
//                                extension keys; construction then throws (the library's refusal on a GPU, the device's error without one).
//   host_fused_bf16_test         (tests/test_gpu_fused_bf16.py): the same, and the throw is the library's refusal of bf16 on the reference's 2 x 64 networks;
//                                then PPO_HostEnvBox at obs_size 100, action_dim 3, hidden_size 128 with fused_policy, wide_obs, matrix_cores and the key is
//                                constructed: the context carries the dtype and the three flags (tests/test_gpu_fused_bf16.py runs the kernels).
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../PPO/PPO_Discrete.h"
#include "../PPO/PPO_HostEnvBox.h"

#define REQUIRE(x) do { if (!(x)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static const int N = 16, T = 32, D = 3, O = 100;

// the smallest env PPO_HostEnvBox takes: a fixed 100-wide observation, no reward, episodes of 8 steps
struct FlatEnv {
    explicit FlatEnv(int64_t) {}
    std::vector<float> reset() { episode_length = 0; episode_reward = 0.0f; return std::vector<float>(O, 0.25f); }
    std::tuple<std::vector<float>, float, bool, bool> step(const std::vector<float>&) { episode_length++; return { std::vector<float>(O, 0.25f), 0.0f, episode_length >= 8, false }; }
    int64_t episode_length = 0;
    float episode_reward = 0.0f;
};

static void writeConfig(const std::string& environment, const std::string& network) {
    std::ofstream f("PPOConfig.toml");
    f << "[environment]\n" << environment << "[network]\n" << network << "bf16 = true\n"
      << "[general]\nseed = 3\ntotal_timesteps = " << N * T << "\nuse_cuda = true\ncheckpoint_updates = 1\n"
         "[ppo]\nlearning_rate = 0.001\nnum_envs = " << N << "\nnum_steps = " << T << "\nanneal_lr = true\nuse_gae = true\ngamma = 0.98\n"
         "gae_lambda = 0.95\nnum_minibatches = 4\nupdate_epochs = 4\nnorm_adv = true\nclip_coef = 0.2\nclip_vloss = true\n"
         "ent_coef = 0.01\nvf_coef = 0.5\nmax_grad_norm = 0.5\n";
}

// what fn prints, also when it throws (the message goes to `threw`)
template <class Fn> static std::string captured(Fn fn, std::string* threw = nullptr) {
    std::stringstream out;
    std::streambuf* old = std::cout.rdbuf(out.rdbuf());
    try { fn(); } catch (const std::exception& e) { std::cout.rdbuf(old); if (!threw) throw; *threw = e.what(); return out.str(); }
    std::cout.rdbuf(old);
    return out.str();
}

int main(int argc, char** argv) {
    const bool parse_only = argc > 1 && std::strcmp(argv[1], "parse") == 0;
    // PPO_Discrete (CartPole on the device): the key is read and printed; no such context exists
    writeConfig("obs_size = 4\naction_size = 2\nmax_episode_steps = 20\n", "");
    std::string refusal = "(nothing was thrown)";
    const std::string said = captured([&] { PPO_Discrete algo; }, &refusal);
    std::printf("refusal: %s\n", refusal.c_str());
    REQUIRE(said.find("Using config file bf16 = true") != std::string::npos && refusal != "(nothing was thrown)");
    std::printf("parsed: bf16 = true\n");
    if (parse_only) return 0;
    REQUIRE(refusal.find("compute_dtype = PPO_DTYPE_BF16") != std::string::npos);

    // PPO_HostEnvBox with fused_policy, wide_obs, matrix_cores and hidden_size = 128: the context carries the dtype and the three flags
    writeConfig("obs_size = " + std::to_string(O) + "\naction_dim = " + std::to_string(D) + "\nmax_episode_steps = 40\nfused_policy = true\nwide_obs = true\n"
                "matrix_cores = true\n", "hidden_size = 128\n");
    using Algo = PPO_HostEnvBox<FlatEnv>;
    std::unique_ptr<Algo> algo;
    const std::string box = captured([&] { algo = std::make_unique<Algo>([](int64_t i) { return std::make_shared<FlatEnv>(i); }); });
    REQUIRE(box.find("Using config file bf16 = true") != std::string::npos && algo->actionDim() == D);
    ppo_config cfg{};
    cfg.struct_size = sizeof cfg;
    REQUIRE(ppo_get_config(algo->m_ctx, &cfg) == PPO_OK);
    REQUIRE(cfg.hidden == 128 && cfg.n_hidden == 2 && cfg.compute_dtype == PPO_DTYPE_BF16);
    REQUIRE(cfg.kernel_flags == (PPO_KERNEL_GAUSS_FUSED | PPO_KERNEL_FUSED_WIDE_OBS | PPO_KERNEL_FUSED_MATRIX));
    std::printf("host_fused_bf16_test ok\n");
    return 0;
}
