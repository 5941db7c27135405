// Type-check stand-in (see ../../README.md).
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>
#include "std_msgs/msg/header.hpp"
namespace sensor_msgs::msg {
struct CompressedImage {
  using SharedPtr = std::shared_ptr<CompressedImage>;
  std_msgs::msg::Header header;
  std::string format;
  std::vector<uint8_t> data;
};
}  // namespace sensor_msgs::msg
